/*
 * scorp_gs.h — C ABI of libscorp_gs.so, the MI355X (gfx950) Gaussian-splat rasterization backend.
 *
 * This is the drop-in boundary for the one hot path of PolySummit/SCORP: everything below
 * `GaussianRasterizer(raster_settings)(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
 * cov3D_precomp)` in gs3dgs/gaussian_renderer/__init__.py:51-66,101-111 (and its 2DGS twin,
 * gs2dgs/gaussian_renderer/__init__.py:51-67,111-120) plus `simple_knn._C.distCUDA2`
 * (gs3dgs/scene/gaussian_model.py:22,177).  The reference binds those through three third-party CUDA torch
 * extensions (`diff_gaussian_rasterization`, `diff_surfel_rasterization`, `simple_knn`; .gitmodules:7-17)
 * whose source is not in the reference tree, so there is no upstream C signature to match: the entry points
 * below are what a ctypes / pybind / cgo binding for this path binds instead.  Plain C: raw device pointers,
 * ints and floats; no torch or pybind types.
 *
 * Conventions (all fixed by the reference's call site):
 *   - every array is fp32, contiguous, resident on the current HIP device, owned by the caller;
 *   - matrices are the 16 floats of the *transposed* 4x4 the reference stores (row-vector convention,
 *     gs3dgs/scene/cameras.py:82-97), i.e. element [r][c] of the maths matrix is m[c*4 + r];
 *   - quaternions are (w,x,y,z) and already normalised by the caller (gaussian_model.py:131-132);
 *   - cov3D_precomp is xx,xy,xz,yy,yz,zz (gs3dgs/utils/general_utils.py:79-88);
 *   - shs is [N, sh_coeffs, 3]; only the first (sh_degree+1)^2 coefficients are read;
 *   - exactly one of {shs, colors_precomp} and one of {scales+rotations, cov3D_precomp} is non-NULL;
 *   - outputs: color[3,H,W] (background composited), depth[1,H,W] = sum z*alpha*T (NOT normalised: the caller
 *     divides by alpha, gaussian_renderer/__init__.py:113), alpha[1,H,W] = sum alpha*T, radii[N] int32.
 *
 * Threading: re-entrant; all work is enqueued on the stream passed in; the only host synchronisation is in
 * scorp_gs3d_num_pairs().  Errors: 0 = ok, negative = failure with a message in scorp_last_error()
 * (thread-local).  With `debug` set every kernel is followed by a stream sync + error check
 * (the reference's `pipe.debug`, gaussian_renderer/__init__.py:63).
 *
 * Style: the Python binding (scorp_amd/_C.py) is derived from this text by a reader that is no C parser and refuses what it
 * does not know, so keep to what is here: block comments only; one declaration per `;`; scalars spelled int, int32_t,
 * uint32_t, int64_t, uint64_t, size_t, float, double; pointers to those, to void, uint8_t or a struct declared above;
 * `#define SCORP_<NAME> <literal>` with the literal written 4, 4u, (-4) or 0.3f.  No function pointers, no unions, no
 * bit-fields, no nested structs by value, no macros in declarations.
 */
#ifndef SCORP_GS_H
#define SCORP_GS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *scorp_stream_t; /* a hipStream_t (NULL = the default stream) */

#define SCORP_OK 0
#define SCORP_ERR_INVALID (-1)   /* bad argument (NULL, size, shape) */
#define SCORP_ERR_HIP (-2)       /* a HIP call or kernel failed */
#define SCORP_ERR_OVERFLOW (-3)  /* the pair buffer was smaller than the number of (tile,splat) pairs */
#define SCORP_ERR_NO_INLIERS (-4) /* scorp_pose_ransac: the best hypothesis has fewer than 3 inliers */

/* The 12 fields of GaussianRasterizationSettings (gaussian_renderer/__init__.py:51-64) + the 8 call arguments. */
typedef struct ScorpGs3dInputs {
  int32_t num_gaussians;    /* N */
  int32_t sh_degree;        /* active degree, 0..3 */
  int32_t sh_coeffs;        /* coefficients allocated per Gaussian in `shs` (= (max_sh_degree+1)^2) */
  int32_t image_width;
  int32_t image_height;
  float tanfovx;
  float tanfovy;
  float scale_modifier;
  int32_t prefiltered;      /* accepted for signature parity; the reference always passes False */
  int32_t debug;
  const float *bg;          /* [3]  device */
  const float *viewmatrix;  /* [16] device */
  const float *projmatrix;  /* [16] device */
  const float *campos;      /* [3]  device */
  const float *means3D;     /* [N,3] */
  const float *shs;         /* [N,sh_coeffs,3] or NULL */
  const float *colors_precomp; /* [N,3] or NULL */
  const float *opacities;   /* [N] (the reference passes [N,1]) */
  const float *scales;      /* [N,3] or NULL */
  const float *rotations;   /* [N,4] or NULL */
  const float *cov3D_precomp; /* [N,6] or NULL */
  /* ---- optional "raw parameter" convention (zero / NULL = the reference call-site convention above) ----
   * The GaussianModel stores logit opacity, log scale, an un-normalised quaternion and the SH coefficients split
   * into _features_dc[N,1,3] / _features_rest[N,K-1,3]; its properties activate and torch.cat them on every view
   * (gs3dgs/scene/gaussian_model.py:126-146).  With these fields the kernels do that themselves and the backward
   * returns gradients w.r.t. the raw values, so the training harness skips six elementwise/cat kernels per view. */
  const float *shs_rest;    /* non-NULL: `shs` is [N,1,3] (degree 0) and shs_rest is [N,sh_coeffs-1,3] */
  int32_t raw_params;       /* bit 0: opacities are logits (sigmoid); bit 1: scales are logs (exp); bit 2: rotations
                               are un-normalised (x / max(|x|, 1e-12)) */
  /* ---- optional: V views of the SAME Gaussians in one launch set (0 or 1 = one view, the reference's call) ----
   * The align loop renders one object from ~15 cameras per pose hypothesis, forward only
   * (align_3dgs_clpe_9dof.py:157-169,336-368); 100 k Gaussians at 800x800 cannot fill the chip, so a single view is a
   * chain of launch-latency-bound kernels.  With num_views = V > 1: viewmatrix / projmatrix / campos are arrays of V
   * entries ([V,16], [V,16], [V,3]), image_height is the height of ONE view (a multiple of 16) and every per-view size
   * is multiplied by V: the V images are rendered as one image of V * image_height rows (view v = rows
   * [v * image_height, (v + 1) * image_height)), Gaussian i of view v is "virtual Gaussian" v * N + i.  So
   * out_radii is [V * N], color [3, V * H, W], the 3DGS depth / alpha [V * H, W] and the 2DGS allmap [7, V * H, W];
   * state / pairs are sized with scorp_gs3d_state_bytes / scorp_gs2d_state_bytes(V * N, W, V * H).  Both kinds read the
   * field, with the same limits: V * N <= 2^31 - 1, V * H <= 16 * 65535, and the stacked image must stay on the LDS
   * binning.  2DGS additionally refuses V > 1 with cov3D_precomp (a given splat->pixel transform belongs to one view).
   * Forward only: scorp_gs3d_render / scorp_gs2d_render and scorp_gs3d_backward* / scorp_gs2d_backward* refuse such
   * inputs; *_preprocess, *_render_image and *_render_score take them. */
  int32_t num_views;
} ScorpGs3dInputs;

/* Gradients w.r.t. the 8 call arguments; any pointer may be NULL (not wanted). Each is fully overwritten. */
typedef struct ScorpGs3dGrads {
  float *means3D;        /* [N,3] */
  float *means2D;        /* [N,3]: (dL/dndc_x, dL/dndc_y, 0) — consumed by add_densification_stats, gaussian_model.py:603-605 */
  float *shs;            /* [N,sh_coeffs,3] */
  float *colors_precomp; /* [N,3] */
  float *opacities;      /* [N] */
  float *scales;         /* [N,3] */
  float *rotations;      /* [N,4] */
  float *cov3D_precomp;  /* [N,6] */
  float *shs_rest;       /* [N,sh_coeffs-1,3] when the forward was given shs_rest (then `shs` is [N,1,3]) */
} ScorpGs3dGrads;

int scorp_version(void);
/* First 16 hex digits of the sha256 over the kernel sources (csrc/ *.hip, *.hpp, this header) the library was built
 * from; profiles/traffic.json and profiles/valu_mix.json carry the same stamp. */
const char *scorp_source_sha(void);
const char *scorp_last_error(void);

/* ---- workspace sizing (pure host arithmetic) ---- */
/* Forward state: per-Gaussian projected records, per-tile ranges, per-pixel final-T / last-contributor. */
size_t scorp_gs3d_state_bytes(int32_t num_gaussians, int32_t image_width, int32_t image_height);
/* Pair buffer for `capacity` (tile,splat) pairs: unsorted 64-bit keys + the depth-sorted 32-bit splat list.  After the
 * sort the key region is reused by the render for one byte per (8x8 pixel block, list entry): whether the splat's
 * footprint reaches the block.  The backward replays exactly those entries, so it must get the SAME pair buffer the
 * render filled (it only reads it). */
size_t scorp_gs3d_pairs_bytes(uint64_t capacity);
/* Scratch of one backward call (per-Gaussian screen-space gradient accumulators), plus the nine planes of
 * ceil(num_gaussians / 256) * 256 floats in which scorp_gs3d_train_view hands d(colour)/d(view direction) from its
 * forward to its backward (see scorp_gs3d_backward_scratch_bytes_ex). */
size_t scorp_gs3d_backward_scratch_bytes(int32_t num_gaussians);

/* ---- forward, in three steps so the caller owns every allocation ---- */
/* 1. project + cull every Gaussian, count splats per tile, prefix-sum the counts. Enqueue only.
 *    Writes radii[N]. `state` must be scorp_gs3d_state_bytes() large and 256-byte aligned. */
int scorp_gs3d_preprocess(const ScorpGs3dInputs *in, int32_t *out_radii, void *state, size_t state_bytes,
                          scorp_stream_t stream);
/* 2. number of (tile,splat) pairs of the preprocess just enqueued. Synchronises the stream (one 8-byte D2H).
 *    A caller that sizes the pair buffer from a previous view may skip this and check
 *    scorp_gs3d_check_overflow() later instead. */
int scorp_gs3d_num_pairs(const void *state, scorp_stream_t stream, uint64_t *num_pairs);
/* 3. bucket pairs by tile, depth-sort each tile, blend front to back. Enqueue only. If the pair buffer is too
 *    small nothing is written out of bounds, outputs are undefined and scorp_gs3d_check_overflow() reports it. */
int scorp_gs3d_render(const ScorpGs3dInputs *in, void *state, void *pairs, uint64_t capacity, float *out_color,
                      float *out_depth, float *out_alpha, scorp_stream_t stream);
/* 3'. the same images with nothing left behind for scorp_gs3d_backward (no per-pixel state, no cull verdicts in the
 *     pair buffer): for the calls the reference makes under torch.no_grad() (align_3dgs_clpe_9dof.py:157-169 scoring
 *     renders, evaluation views).  Same arguments, same outputs bit for bit. */
int scorp_gs3d_render_image(const ScorpGs3dInputs *in, void *state, void *pairs, uint64_t capacity, float *out_color,
                            float *out_depth, float *out_alpha, scorp_stream_t stream);
/* 3''. render-and-compare in one: step 3 for a caller that only wants to know how far the render is from a target (the
 *      rotation sweep's scoring, align_3dgs_clpe_9dof.py:80-111 / :336-368, as scorp_gs3d_pose_score_accumulate defines it).
 *      No image is written and no colour accumulated; the image's rows are cut into bands of rows_per_score rows (a
 *      multiple of 16 dividing the image height - with num_views = V stacked views: V * image_height, or a multiple of it
 *      when several hypotheses share the launch), every band is compared with the SAME target tgt_depth / tgt_alpha
 *      [rows_per_score, W] (tgt_depth normalised, as scorp_gs3d_render_tail writes it), and
 *        acc[j] += scale * sum over band j of |alpha - tgt_alpha| + |nan_to_num(depth / alpha, 0, 0) - tgt_depth|.
 *      The per-block partial sums are added in a fixed order: two runs give the same bits. */
int scorp_gs3d_render_score(const ScorpGs3dInputs *in, void *state, void *pairs, uint64_t capacity, const float *tgt_depth,
                            const float *tgt_alpha, int32_t rows_per_score, float scale, float *acc, scorp_stream_t stream);
/* Synchronises; returns SCORP_ERR_OVERFLOW if the last render on this state needed more than `capacity` pairs
 * (and the needed count in *num_pairs), SCORP_OK otherwise. */
int scorp_gs3d_check_overflow(const void *state, scorp_stream_t stream, uint64_t *num_pairs);

/* ---- backward ---- */
/* `state` and `pairs` are the buffers of the matching forward and are only READ, so several backward passes
 * may run on one forward (utils/mask.py:52,65,89 does). dL_dcolor[3,H,W]; dL_ddepth / dL_dalpha [H,W] or NULL. */
int scorp_gs3d_backward(const ScorpGs3dInputs *in, const void *state, const void *pairs, uint64_t capacity,
                        const float *dL_dcolor, const float *dL_ddepth, const float *dL_dalpha,
                        const ScorpGs3dGrads *grads, void *scratch, size_t scratch_bytes, scorp_stream_t stream);
/* The same with `flags`.  The blend backward reduces over a block's pixels on the matrix cores; by default the two
 * factors travel as two fp16 terms each (22 bits, exact products, fp32 accumulation: "split" form, the fast one).
 * SCORP_BACKWARD_EXACT_FP32 selects fp32 MFMAs throughout (the form the reference CUDA's fp32 arithmetic corresponds
 * to; ~1.3x the blend-backward time): the parity tests compare the two.  scorp_gs3d_backward == flags 0. */
#define SCORP_BACKWARD_EXACT_FP32 1u
/* SCORP_BACKWARD_SCRATCH_ZEROED: the caller guarantees that the first num_gaussians * 64 bytes of `scratch` (the
 * per-Gaussian accumulator rows) are zero when the call starts, so the library skips its 64 MB-per-million fill.
 * scorp_gs3d_train_view uses it: there the blend FORWARD's waves, whose memory pipes idle, clear the rows on the way. */
#define SCORP_BACKWARD_SCRATCH_ZEROED 2u
/* SCORP_BACKWARD_DETERMINISTIC: no float atomics.  Every (8x8 block, hit) writes its ten sums as one plain 64-byte row
 * partial[4 * pair + block], pair = the ordinal of its (Gaussian, tile) pair in Gaussian-major order (an exclusive scan of
 * the Gaussians' tile counts + the tile's rank in the Gaussian's tile mask), with one flag byte per row; a second kernel
 * then adds, per Gaussian, its rows - contiguous by construction - in a FIXED order: its tiles in mask order, the four
 * blocks of a tile in order.  Two runs on the same inputs give the same bits: `get_mask3d` votes on the SIGN of repeated
 * backward passes on one forward (utils/mask.py:52,65,89,124), which atomic accumulation order can flip for sums near
 * zero.  Needs the larger scratch of scorp_gs3d_backward_scratch_bytes_ex. */
#define SCORP_BACKWARD_DETERMINISTIC 4u
/* scratch size for scorp_gs3d_backward_ex with `flags`: the accumulator rows (num_gaussians * 64 bytes), plus, for
 * SCORP_BACKWARD_DETERMINISTIC, num_gaussians + 1 pair ordinals, 4 * capacity flag bytes and 4 * capacity rows of 64 bytes.
 * Behind that, 9 * ceil(num_gaussians / 256) * 256 floats that only scorp_gs3d_train_view[_ex] uses: with the training
 * layout at SH degree 3 its per-Gaussian forward leaves d(colour)/d(view direction) there and its backward reads these
 * nine floats per Gaussian instead of the SH rows.  Every call accepts a buffer without that tail (this size minus
 * 36 * ceil(num_gaussians / 256) * 256 bytes); the view then reads the rows a second time, with the same results. */
size_t scorp_gs3d_backward_scratch_bytes_ex(int32_t num_gaussians, int32_t image_width, int32_t image_height, uint64_t capacity,
                                            uint32_t flags);
int scorp_gs3d_backward_ex(const ScorpGs3dInputs *in, const void *state, const void *pairs, uint64_t capacity,
                           const float *dL_dcolor, const float *dL_ddepth, const float *dL_dalpha,
                           const ScorpGs3dGrads *grads, void *scratch, size_t scratch_bytes, uint32_t flags,
                           scorp_stream_t stream);

/* ---- 3-D segmentation by 2-D object masks (utils/mask.py:42-124 get_mask3d, one pass instead of 1 + 2K backwards) ----
 * With w_i(p) = alpha_i(p) T_i(p) the blend weight the render gave Gaussian i at pixel p (zero where it was not blended) and
 * masks[k][p] != 0 meaning "p is inside object k":
 *   S_in[k][i] = sum over the pixels inside mask k of w_i(p),   S_out[k][i] = the same sum over the pixels outside it.
 * One front-to-back replay of the hit lists scorp_gs3d_render / scorp_gs2d_render left (alpha recomputed with the forward's
 * own arithmetic), eight objects per pass over the view; no float atomics, so two calls give the same bits.  The result is
 * ADDED into `out` (views accumulate).  `masks` is [num_masks, H, W] bytes on the device, `out` fp32 on the device:
 *   SCORP_VOTE_SUMS      out[K, 2, N]: out[k][0][i] += S_in, out[k][1][i] += S_out
 *   SCORP_VOTE_GRADIENT  out[K, N]:    out[k][i] += scale * (S_in - S_out)   (get_mask3d's "gradient": scale = 1 / (sqrt(3) H W))
 *   SCORP_VOTE_BINARY    out[K, N]:    out[k][i] += (S_in > 0) - (S_out > 0)
 * Valid after *_preprocess + *_render (NOT after *_render_image / *_render_score, which leave no hit lists; the state cannot
 * tell, and the result is then undefined); `capacity` is the one the render ran with.  The state and the pair buffer are
 * only read: a backward after a vote gives the same bits as one without it.  Synchronises once (reads the state header).
 * SCORP_ERR_INVALID: num_masks < 1, a NULL pointer, num_views > 1, an unknown method, scratch too small (or not 256-byte
 * aligned), a capacity other than the render's; SCORP_ERR_OVERFLOW: the render overflowed its pair buffer.  N = 0 or an
 * empty image: nothing is done. */
#define SCORP_VOTE_SUMS 0u
#define SCORP_VOTE_GRADIENT 1u
#define SCORP_VOTE_BINARY 2u
size_t scorp_mask_vote_scratch_bytes(int32_t num_gaussians, int32_t image_width, int32_t image_height, uint64_t capacity);
int scorp_gs3d_mask_vote(const ScorpGs3dInputs *in, const void *state, const void *pairs, uint64_t capacity,
                         const uint8_t *masks, int32_t num_masks, uint32_t method, float scale, float *out, void *scratch,
                         size_t scratch_bytes, scorp_stream_t stream);
/* The same on a scorp_gs2d_preprocess + scorp_gs2d_render state. */
int scorp_gs2d_mask_vote(const ScorpGs3dInputs *in, const void *state, const void *pairs, uint64_t capacity,
                         const uint8_t *masks, int32_t num_masks, uint32_t method, float scale, float *out, void *scratch,
                         size_t scratch_bytes, scorp_stream_t stream);

/* ---- multi-start point-to-point ICP (align_3dgs_clpe_9dof.py:42-115 get_ICP_fitting_transformation_best: Open3D
 * registration_icp with TransformationEstimationPointToPoint, no scaling, from every init of a batch) ----
 * source[n_source, 3], target[n_target, 3] fp32 and inits[n_init, 4, 4] row-major float64 (rigid: last row 0 0 0 1) are
 * device pointers, as are the outputs: out_transformation[n_init, 4, 4] float64, out_fitness / out_inlier_rmse[n_init]
 * float64, out_iterations[n_init] int32.  Per init, with r = max_correspondence_distance:
 *   pass(T):   x = T p for every source point; its pair is the nearest target point q with |x - q|^2 <= r^2 (exact search;
 *              ties: the lower target index); c pairs, fitness = c / n_source, inlier_rmse = sqrt(sum |x - q|^2 / c)
 *              (both 0 when c = 0);
 *   update:    Umeyama / Kabsch without scale on the pairs (R = U D V^T, D = diag(1, 1, -1) iff det U det V < 0,
 *              t = qm - R xm; the identity when c = 0);
 *   loop:      result_0 = pass(T_0); for i < max_iteration: T_{i+1} = update(result_i) T_i, result_{i+1} = pass(T_{i+1}),
 *              stop when |d fitness| < relative_fitness AND |d rmse| < relative_rmse.
 * The outputs are the last T with its fitness and rmse, and the number of updates made.  The search runs in fp32
 * relative to the target's bounding-box centre; the pair test, d^2 and the moments are float64, the transforms are
 * composed in float64 and always applied to the original points.  No float atomics: two calls give the same bits, and an
 * init run alone gives the bits it gets in a batch.  The inputs are only read.  workspace: scorp_icp_workspace_bytes,
 * 256-byte aligned.  Synchronises every few iterations (reads the per-init active flags) and returns when every init has
 * stopped.  SCORP_ERR_INVALID: r <= 0 (or not finite), an empty cloud, max_iteration < 0, n_init outside [1, 65535], a
 * NULL pointer, a workspace too small or misaligned. */
size_t scorp_icp_workspace_bytes(int32_t n_source, int32_t n_target, int32_t n_init);
int scorp_icp_point_to_point(const float *source, int32_t n_source, const float *target, int32_t n_target,
                             const double *inits, int32_t n_init, double max_correspondence_distance, int32_t max_iteration,
                             double relative_fitness, double relative_rmse, double *out_transformation, double *out_fitness,
                             double *out_inlier_rmse, int32_t *out_iterations, void *workspace, size_t workspace_bytes,
                             scorp_stream_t stream);

/* ---- multi-start point-to-plane ICP (Open3D registration_icp with TransformationEstimationPointToPlane, no robust
 * kernel, from every init of a batch) ----
 * Inputs, outputs, pass(T), the loop, the stop rule, the precision of the search (fp32 relative to c_t, the centre of the
 * target's bounding box; everything after it float64), the determinism and the error codes are those of
 * scorp_icp_point_to_point; inlier_rmse stays the Euclidean sqrt(sum |x - q|^2 / c).  target_normals[n_target, 3] fp32
 * (device) is added: the normal n of target point q.  Normals are used as given, not normalised; a zero normal adds
 * nothing to the update (its pair still counts in fitness and inlier_rmse).  A NULL target_normals is SCORP_ERR_INVALID.
 *   update:    from the c pairs (x, q, n) of a pass, every coordinate relative to c_t, with s = half the largest edge of
 *              the target's bounding box (1 if that is 0):
 *                J = [(x cross n) / s ; n] in R^6, rho = n . (x - q), A = sum J J^T, b = sum J rho;
 *                A = V L V^T (cyclic Jacobi, float64);
 *                xi = - sum over { l_i > 1e-12 l_max } of v_i (v_i . b) / l_i   (the minimum-norm step: a rank-deficient
 *                     system - a planar target, one pair - moves only along the directions it constrains);
 *                xi = 0, the identity, when c = 0 or l_max = 0;
 *                omega = xi[0:3] / s, tau = xi[3:6], R = Rz(omega_z) Ry(omega_y) Rx(omega_x);
 *              the update is x' -> R x' + tau about c_t, in absolute terms [R | tau + c_t - R c_t], composed onto T.
 * workspace: scorp_icp_point_to_plane_workspace_bytes, 256-byte aligned. */
size_t scorp_icp_point_to_plane_workspace_bytes(int32_t n_source, int32_t n_target, int32_t n_init);
int scorp_icp_point_to_plane(const float *source, int32_t n_source, const float *target, const float *target_normals,
                             int32_t n_target, const double *inits, int32_t n_init, double max_correspondence_distance,
                             int32_t max_iteration, double relative_fitness, double relative_rmse,
                             double *out_transformation, double *out_fitness, double *out_inlier_rmse,
                             int32_t *out_iterations, void *workspace, size_t workspace_bytes, scorp_stream_t stream);

/* ---- multi-start generalized ICP (Segal, Haehnel, Thrun 2009; what Open3D's registration_generalized_icp is used for:
 * two independent samplings of one surface, every point with a covariance; from every init of a batch) ----
 * Open3D could not be run where this was written: the rules below ARE the specification.
 * Inputs, outputs, pass(T), the loop, the stop rule, the precision of the search, the determinism and the error codes are
 * those of scorp_icp_point_to_point; inlier_rmse stays the Euclidean sqrt(sum |x - q|^2 / c).  source_covariances
 * [n_source, 6] and target_covariances[n_target, 6] fp32 (device) are added: the upper triangle xx, xy, xz, yy, yz, zz of
 * the covariance C_p of source point p and C_q of target point q.  They are used as given, not normalised and not
 * regularised.  A NULL covariance pointer is SCORP_ERR_INVALID.
 *   update:    from the c pairs (x, q, C_p, C_q) of a pass, in float64, every coordinate relative to c_t, with s as for
 *              point-to-plane and A_T the upper-left 3x3 of the init's cumulative T as stored:
 *                u = x - q, M = C_q + A_T C_p A_T^T (symmetric, from the six values of each covariance);
 *                a pair enters the update only if M is finite and positive definite by Sylvester's test (M00 > 0,
 *                M00 M11 - M01^2 > 0, det M > 0); any other pair adds nothing to A and b (it still counts in c, fitness
 *                and inlier_rmse, as a zero normal does for point-to-plane);
 *                W = M^-1 by cofactors over det M, J = [ -[x]x / s | I ] (3 x 6),
 *                A = sum J^T W J, b = sum J^T W u = sum [ (x cross (W u)) / s ; W u ];
 *              everything after that is the point-to-plane update unchanged: Jacobi on A, the minimum-norm step over the
 *              eigenvalues above 1e-12 l_max, the identity when c = 0 or l_max = 0, omega = xi[0:3] / s, tau = xi[3:6],
 *              R = Rz Ry Rx, composed about c_t.  With W = n n^T these are the point-to-plane sums term for term.
 * workspace: scorp_icp_generalized_workspace_bytes (the point-to-plane workspace and the source's covariances in its
 * sorted order), 256-byte aligned. */
size_t scorp_icp_generalized_workspace_bytes(int32_t n_source, int32_t n_target, int32_t n_init);
int scorp_icp_generalized(const float *source, const float *source_covariances, int32_t n_source, const float *target,
                          const float *target_covariances, int32_t n_target, const double *inits, int32_t n_init,
                          double max_correspondence_distance, int32_t max_iteration, double relative_fitness,
                          double relative_rmse, double *out_transformation, double *out_fitness, double *out_inlier_rmse,
                          int32_t *out_iterations, void *workspace, size_t workspace_bytes, scorp_stream_t stream);

/* ---- multi-start coloured ICP (Park, Zhou, Koltun 2017; what Open3D's registration_colored_icp is used for: surfaces
 * that slide or spin at no geometric cost and carry a texture; from every init of a batch) ----
 * Open3D could not be run where this was written: the rules below ARE the specification.
 * Inputs, outputs, pass(T), the loop, the stop rule, the precision of the search, the determinism and the error codes are
 * those of scorp_icp_point_to_point; fitness and inlier_rmse stay those of the pairs' positions (the Euclidean
 * sqrt(sum |x - q|^2 / c): the colour residual does not enter them).  The arguments are those of
 * scorp_icp_point_to_plane, plus source_intensity[n_source], target_intensity[n_target] and target_gradients[n_target, 3]
 * fp32 (device; scorp_color_gradients makes the last) and lambda_geometric in [0, 1].  All are used as given.
 *   update:    from the c pairs of a pass - x, q, the normal n, the gradient d and the intensity I_q of q, the intensity I_p
 *              of the source point - in float64, every coordinate relative to c_t, with s as for point-to-plane:
 *                rho_G = n . (x - q),               J_G = [(x cross n) / s ; n],
 *                rho_C = d . (x - q) + (I_q - I_p), J_C = [(x cross d) / s ; d],
 *                A = sum lambda J_G J_G^T + (1 - lambda) J_C J_C^T,
 *                b = sum lambda J_G rho_G + (1 - lambda) J_C rho_C;
 *              everything after that is the point-to-plane update unchanged: Jacobi on A, the minimum-norm step over the
 *              eigenvalues above 1e-12 l_max, the identity when c = 0 or l_max = 0, omega = xi[0:3] / s, tau = xi[3:6],
 *              R = Rz Ry Rx, composed about c_t.
 * Because d is tangent, d . (x - q) is the gradient applied to the projection of x into the tangent plane of q: there is
 * no separate projection step.  A zero normal contributes only its colour term, a zero gradient with equal intensities
 * only its geometric term; either way the pair counts in c.  Constant colour, or lambda = 1, gives the point-to-plane step.
 * SCORP_ERR_INVALID as for scorp_icp_point_to_plane, and: lambda_geometric outside [0, 1] or not finite, a NULL pointer
 * among the new ones.  workspace: scorp_icp_colored_workspace_bytes (the point-to-plane workspace and the source's
 * intensities in its sorted order), 256-byte aligned. */
size_t scorp_icp_colored_workspace_bytes(int32_t n_source, int32_t n_target, int32_t n_init);
int scorp_icp_colored(const float *source, const float *source_intensity, int32_t n_source, const float *target,
                      const float *target_normals, const float *target_intensity, const float *target_gradients,
                      int32_t n_target, const double *inits, int32_t n_init, double max_correspondence_distance,
                      int32_t max_iteration, double relative_fitness, double relative_rmse, double lambda_geometric,
                      double *out_transformation, double *out_fitness, double *out_inlier_rmse, int32_t *out_iterations,
                      void *workspace, size_t workspace_bytes, scorp_stream_t stream);

/* Normals of a cloud that brings none (3DGS centres).  points[n, 3] fp32, out_normals[n, 3] fp32 and the optional
 * out_neighbors[n, knn] int32 (NULL: skipped) are device pointers.  Per point:
 *   neighbours: its k = min(knn, n) exact nearest points, itself included, ordered by (d^2, index): ties go to the lower
 *               index.  The search runs on the uniform grid of the ICP calls, in fp32 relative to the centre of the
 *               cloud's bounding box.  out_neighbors holds them in that order, padded with -1 when knn > n;
 *   normal:     the float64 covariance of the k neighbours about their mean, the eigenvector of its smallest eigenvalue
 *               (3x3 Jacobi, float64), scaled to unit length, signed so that its component of largest magnitude (the
 *               first of equal ones) is positive.  n < 3: (0, 0, 1).
 * The normals are not oriented (inside / outside): point-to-plane ICP does not depend on the sign.  No atomics: two calls
 * give the same bits.  The input is only read.  workspace: scorp_estimate_normals_workspace_bytes(n), 256-byte aligned.
 * SCORP_ERR_INVALID: knn outside [3, 32], an empty cloud, a NULL points / out_normals / workspace, a workspace too small
 * or misaligned. */
size_t scorp_estimate_normals_workspace_bytes(int32_t n);
int scorp_estimate_normals(const float *points, int32_t n, int32_t knn, float *out_normals, int32_t *out_neighbors,
                           void *workspace, size_t workspace_bytes, scorp_stream_t stream);

/* Colour gradients of a cloud, for scorp_icp_colored.  points[n, 3], normals[n, 3], intensity[n] fp32, neighbors[n, knn]
 * int32 in the layout scorp_estimate_normals writes (sorted, padded with -1) and out_gradients[n, 3] fp32 are device
 * pointers; knn in [3, 32].  Per point i, in float64:
 *   nh = n_i / |n_i|; nh = 0 for a zero or non-finite normal (nothing is projected out);
 *   over the row's entries j >= 0, j != i, in row order (an entry >= n is skipped):
 *     u_j = p_j - p_i, e_j = u_j - (u_j . nh) nh, delta_j = I_j - I_i;
 *   M = sum e_j e_j^T + (sum |e_j|^2) nh nh^T, g = sum e_j delta_j;
 *   M = V L V^T (3x3 Jacobi, float64);
 *   d = sum over { l_k > 1e-12 l_max } of v_k (v_k . g) / l_k;
 *   d = 0 when fewer than two neighbours were used or l_max = 0;
 *   d is rounded to fp32 on the store.
 * The second term of M keeps d in the tangent plane (d . nh = 0 up to rounding) and M well-conditioned wherever the
 * neighbours span that plane; collinear neighbours give the component along their line and nothing else.  One thread per
 * point, no atomics: two calls give the same bits.  The inputs are only read.  No workspace.  SCORP_ERR_INVALID: knn outside
 * [3, 32], an empty cloud, more than 2^30 points, a NULL pointer. */
int scorp_color_gradients(const float *points, const float *normals, const float *intensity, const int32_t *neighbors,
                          int32_t n, int32_t knn, float *out_gradients, scorp_stream_t stream);

/* ---- cleaning a point cloud: k-nearest mean distances, radius counts, DBSCAN (what Open3D's remove_statistical_outlier,
 * remove_radius_outlier and cluster_dbscan are used for; the alignment scripts size their objects by the bounding box of
 * all Gaussian centres, align_3dgs_clpe_9dof.py:377-382, floaters included) ----
 * Open3D could not be run where this was written.  The rules below ARE the specification; nothing was compared with
 * Open3D's own output, and "believed" marks what Open3D is believed, unchecked, to do.  The float64 brute force of
 * tests/cloud_reference.py restates them; its core flags, core partition and noise set equal scikit-learn's
 * DBSCAN(algorithm="brute") and its k-nearest means agree with scipy's cKDTree on the test fixtures.
 *
 * points[n, 3] is float32, finite (the caller's to check), and only read.  Every pointer is a device pointer.  All
 * arithmetic is float64 from the float32 inputs, every product and sum rounded on its own (no fp contraction).
 *
 * R1 distance.    d2(i, j) = (dx dx + dy dy) + dz dz with dx = double(p_i.x) - double(p_j.x) and so on: each difference is
 *                 exact, d2 is symmetric, d2(i, i) = 0.
 * R2 radius.      N_r(i) = { j : d2(i, j) <= radius radius }, radius radius one rounded product: inclusive, and i is a member.
 *                 out_count[i] = |N_r(i)|, exact.
 * R3 k nearest.   k = min(knn, n).  The neighbours of i are the first k points in ascending order of (d2(i, j), j): i itself
 *                 takes part, and a duplicate of lower index comes before it.  out_neighbors[i] holds them in that order,
 *                 padded with -1 when knn > n.  out_mean_distance[i] = (the sum, taken in that order from 0.0, of
 *                 sqrt(d2)) / k.
 * R4 core.        core(i) = |N_eps(i)| >= min_points, i included (scikit-learn's rule; believed to be Open3D's).
 * R5 clusters.    The connected components of the graph on the core points whose edges join core points i, j with j in
 *                 N_eps(i), numbered in ascending order of the smallest core index they contain (the order in which a
 *                 sequential scan opens them).
 * R6 border.      A point that is not core takes the label of the core point of N_eps(i) with the smallest (d2, index), and
 *                 -1 (noise) when there is none.  Open3D and scikit-learn give a border point to whichever cluster reaches
 *                 it first; this rule is a function of the input alone.  out_num_clusters may be 0.
 * R7 determinism. No float atomics.  The union-find hooks a root only under a smaller index (as scorp_mesh_cluster_link):
 *                 two calls give the same bits, every output is a function of the input alone, and permuting the input
 *                 permutes out_count and out_mean_distance exactly.
 * R8 the grid only prunes.  The points are filed into the uniform grid of the ICP calls by their fp32 coordinates relative
 *                 to the centre of the bounding box.  A ring of cells is left unvisited only when every point that can have
 *                 been filed in it is provably outside the radius, or farther than the current k-th distance, the roundings
 *                 of the filing and of the fp32 ring bound allowed for.  Every decision of R2 - R6 is taken on R1's d2 of the
 *                 original coordinates.  A radius far larger than the cell edge h (about one point per cell) makes every
 *                 point visit (2 radius / h)^3 cells: accepted.
 *
 * scorp_cloud_dbscan: out_labels[n] int32, out_core[n] one byte per point (NULL: skipped), out_count[n] = |N_eps(i)|
 * (NULL: skipped), out_num_clusters one int32.  One grid, three walks (count, link, border); no neighbour list is stored.
 * workspace: scorp_cloud_workspace_bytes(n), 256-byte aligned, for all three calls.  None synchronises.
 * SCORP_ERR_INVALID: n < 1 or > 2^30, knn outside [1, 32], radius or eps not positive and finite, min_points < 1, a NULL
 * points / out_mean_distance / out_count (radius call) / out_labels / out_num_clusters, a workspace NULL, too small or
 * misaligned. */
size_t scorp_cloud_workspace_bytes(int32_t n);
int scorp_cloud_knn_distance(const float *points, int32_t n, int32_t knn, double *out_mean_distance, int32_t *out_neighbors,
                             void *workspace, size_t workspace_bytes, scorp_stream_t stream);
int scorp_cloud_radius_count(const float *points, int32_t n, double radius, int32_t *out_count, void *workspace,
                             size_t workspace_bytes, scorp_stream_t stream);
int scorp_cloud_dbscan(const float *points, int32_t n, double eps, int32_t min_points, int32_t *out_labels, uint8_t *out_core,
                       int32_t *out_count, int32_t *out_num_clusters, void *workspace, size_t workspace_bytes,
                       scorp_stream_t stream);

/* ---- global registration from geometry alone: the FPFH descriptor and the nearest-descriptor search (what Open3D's
 * compute_fpfh_feature and registration_ransac_based_on_feature_matching are used for, next to registration_icp;
 * scorp_amd/global_registration.py drives them and hands the matched pairs to scorp_pose_ransac) ----
 * Open3D could not be run where this was written.  The rules below ARE the specification; nothing was compared with
 * Open3D's own output, and "believed, unchecked" marks what Open3D is believed to do.  tests/fpfh_reference.py restates
 * the rules as a float64 brute force.
 *
 * points[n, 3] and normals[n, 3] are float32, finite (the caller's to check) and only read; the normals are used as given
 * and NOT normalised.  All arithmetic is float64 from the float32 inputs, every product and sum rounded on its own (no fp
 * contraction); sqrt and / are correctly rounded.  No float atomics.  Every output is a function of the input alone, and
 * permuting the input permutes the outputs.
 *
 * F1 neighbourhood. d2 is R1 of the cloud block.  N(i) = the first min(max_nn, .) of { j != i : d2(i, j) <= radius radius }
 *                 in ascending (d2, j); radius radius is one rounded product.  i is left out BY INDEX: a duplicate of i is
 *                 a member.  m_i = |N(i)|.  Open3D's hybrid search counts the point itself, so its max_nn is believed,
 *                 unchecked, to be ours + 1.  The grid only prunes (R8).  The list is written once and read by F4 and F5.
 * F2 pair feature of (i, j), j in N(i).  dp = p_j - p_i (each difference exact), f4 = sqrt(d2); f4 = 0 gives no feature.
 *                 dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.  a1 = dot(n_i, dp) / f4, a2 = dot(n_j, dp) / f4.  If
 *                 |a1| < |a2| (strict) then (u, n2, dp, f3) = (n_j, n_i, -dp, -a2), else (u, n2, f3) = (n_i, n_j, a1): Open3D's
 *                 acos(|a1|) > acos(|a2|) stated without acos, believed equivalent, unchecked.  v = dp x u, each component
 *                 a difference of two rounded products; |v| = sqrt(dot(v, v)); |v| = 0 gives no feature (Open3D is
 *                 believed, unchecked, to bin a zero feature instead).  v = v / |v| per component, w = u x v,
 *                 f2 = dot(v, n2), f1 = atan2(dot(w, n2), dot(u, n2)).
 * F3 bins.        b1 = floor((11 (f1 + pi)) / (2 pi)), b2 = floor(11 ((f2 + 1) 0.5)), b3 = floor(11 ((f3 + 1) 0.5)), each
 *                 clamped to [0, 10]; pi is M_PI, 2 pi its exact double.
 * F4 SPFH.        count_i[11 k + b_k] += 1 for k = 0, 1, 2 per pair that has a feature (integers: the order is free).
 *                 spfh_i = count_i (100.0 / m_i): one rounded division, one product per bin; m_i = 0 gives a zero row.
 *                 Pairs without a feature still count in m_i.
 * F5 FPFH.        s = a zero row of 33.  For j in N(i) IN LIST ORDER with d2(i, j) > 0: s[b] = s[b] + spfh_j[b] / d2(i, j).
 *                 For each block k of 11: t = the sum of its entries in ascending order from 0.0; if t != 0 the block's
 *                 entries are multiplied by (100.0 / t).  out_feature[i] = s + spfh_i.
 *
 * scorp_cloud_fpfh: out_feature[n, 33] float64; optional (NULL: kept in the workspace) out_spfh_count[n, 33] int32,
 * out_neighbors[n, max_nn] int32 padded with -1 and out_degree[n] int32 (m_i).  workspace:
 * scorp_cloud_fpfh_workspace_bytes(n, max_nn), 256-byte aligned.  Does not synchronise.  SCORP_ERR_INVALID: n < 1 or
 * > 2^30, radius not positive and finite, max_nn outside [1, 64], a NULL points / normals / out_feature, a workspace NULL,
 * too small or misaligned.
 *
 * M1 match.       src[ns, 33] and tgt[nt, 33] are float32 (the descriptor rounded once by the caller).  D2(a, b) = the sum
 *                 for k = 0 .. 32 in ascending order from 0.0 of (double(a_k) - double(b_k))^2, each difference exact.
 *                 out_index[i] = the target row of smallest (D2, index), out_d2[i] its D2.  (A source row with a NaN has
 *                 no smallest D2: index -1, D2 +inf.)
 * scorp_feature_match: a brute force.  The target's tiles of scorp_feature_match_tile_rows() rows are split over a second
 * grid dimension, scorp_feature_match_split_rows(ns, nt) rows per split, and the splits' bests are merged by the same rule
 * in a second kernel: no atomics.  workspace: scorp_feature_match_workspace_bytes(ns, nt), 256-byte aligned (the splits'
 * partial results).  Does not synchronise.  SCORP_ERR_INVALID: ns or nt < 1 or > 2^30, a NULL pointer, a workspace NULL,
 * too small or misaligned. */
size_t scorp_cloud_fpfh_workspace_bytes(int32_t n, int32_t max_nn);
int scorp_cloud_fpfh(const float *points, const float *normals, int32_t n, double radius, int32_t max_nn, double *out_feature,
                     int32_t *out_spfh_count, int32_t *out_neighbors, int32_t *out_degree, void *workspace,
                     size_t workspace_bytes, scorp_stream_t stream);
int32_t scorp_feature_match_tile_rows(void);
int32_t scorp_feature_match_split_rows(int32_t ns, int32_t nt);
size_t scorp_feature_match_workspace_bytes(int32_t ns, int32_t nt);
int scorp_feature_match(const float *src, int32_t ns, const float *tgt, int32_t nt, int32_t *out_index, double *out_d2,
                        void *workspace, size_t workspace_bytes, scorp_stream_t stream);

/* ---- consistent orientation of a cloud's normals: signs propagated along the minimum spanning forest of the neighbour
 * graph (what Open3D's orient_normals_consistent_tangent_plane is used for; the descriptor above is built from Darboux
 * frames and depends on the sign of every normal).  The rules below ARE the specification and are this project's own:
 * nothing was compared with Open3D, whose Riemannian graph adds the edges of a Euclidean spanning tree; those are not
 * built.  tests/orient_reference.py restates the rules in float64 numpy (Kruskal in O3's order).
 *
 * points[n, 3] and normals[n, 3] are float32, finite (the caller's to check) and only read; the normals are used as given
 * and NOT normalised.  neighbors[n, k] is int32.  Every pointer but `center` is a device pointer.
 *
 * O1 graph.       The vertices are the n points.  {i, j}, i != j, is an edge when j is in row i of the list or i is in row
 *                 j.  1 <= k <= 64.  An entry < 0 is padding, an entry equal to its row index is ignored, duplicates are
 *                 harmless.  An entry >= n is an error that the CALLER rejects before the call (the Python wrapper does and
 *                 raises); the kernels skip such an entry and never follow it.  n <= 2^30.
 * O2 weight.      dot(i, j) = (nx_i nx_j + ny_i ny_j) + nz_i nz_j in float64 on the float32 normals, every product and sum
 *                 rounded on its own (no fp contraction); w = 1 - |dot|.  w may be negative for normals longer than 1.
 * O3 order.       Edges are ordered by (w, min(i, j), max(i, j)), lexicographically: a strict total order, so the minimum
 *                 spanning forest is unique.
 * O4 propagation. Along an edge of the forest the two ends agree when dot >= 0 and are opposite when dot < 0; a dot of
 *                 exactly 0 is not a flip.  rel(x) is the parity of x relative to the smallest index m of its component,
 *                 rel(m) = 0.
 * O5 component sign.  SCORP_ORIENT_MAJORITY_AWAY: c = center[3] (HOST float64, finite), or for a NULL center the float64
 *                 mean of the points by this fixed order of additions: S_g, g < 16384, = the sum from 0.0 of the points
 *                 g, g + 16384, g + 32768, ... in ascending order; T_t, t < 256, = the sum from 0.0 of S_64t .. S_64t+63
 *                 in ascending order; c = (the sum from 0.0 of T_0 .. T_255 in ascending order) / n, per coordinate.  For
 *                 each member with its O4 sign, d = p - c (one rounded difference per coordinate) and
 *                 dd = (n.x d.x + n.y d.y) + n.z d.z in float64; votes = #(dd > 0) - #(dd < 0), counted with integer
 *                 atomics.  The component is flipped when votes < 0; a tie leaves it.  SCORP_ORIENT_FIRST: no vote, m keeps
 *                 its given normal.
 * O6 outputs.     out_normals[n, 3] float32: each row is the input row or its IEEE negation bit for bit (a zero becomes
 *                 -0.0).  Optional (NULL: skipped) out_flip[n] one byte per point, out_label[n] int32 = m, out_tree[n, 2]
 *                 int32 = the forest's edges as (lo, hi), (-1, -1) in unused rows, the order of the rows unspecified.
 *                 out_counts[2] int32 = {components, edges of the forest}.
 *
 * scorp_cloud_orient_normals: Boruvka rounds of four launches (smallest weight per component and smallest (lo, hi) among
 * its edges by two 64-bit atomicMin passes, one hook per root, one compression), ceil(log2 n) + 1 of them launched
 * unconditionally, a round with nothing to do returning on a device flag.  Only integer atomics whose result does not
 * depend on their order: two calls give the same bits and every output is a function of the input alone.  workspace:
 * scorp_cloud_orient_workspace_bytes(n, k), 256-byte aligned.  Does not synchronise and reads nothing back.
 * SCORP_ERR_INVALID: n < 1 or > 2^30, k outside [1, 64], an unknown component_sign, a center that is not finite, a NULL
 * points / normals / neighbors / out_normals / out_counts, a workspace NULL, too small or misaligned. */
#define SCORP_ORIENT_MAJORITY_AWAY 0
#define SCORP_ORIENT_FIRST 1
size_t scorp_cloud_orient_workspace_bytes(int32_t n, int32_t k);
int scorp_cloud_orient_normals(const float *points, const float *normals, const int32_t *neighbors, int32_t n, int32_t k,
                               const double *center, int32_t component_sign, float *out_normals, uint8_t *out_flip,
                               int32_t *out_label, int32_t *out_tree, int32_t *out_counts, void *workspace,
                               size_t workspace_bytes, scorp_stream_t stream);

/* ---- pose fit from matched 3-D point pairs (utils/solution.py: pc_align_ransac :476-557 and adam_algorithm_3d3d_9dof
 * :363-446, called once per round and object by the alignment scripts) ----
 * source[n_pairs, 3] and target[n_pairs, 3] are float64 device pointers, row i of one matched to row i of the other; every
 * output is a device pointer too.  All arithmetic is float64, no float atomics: two calls give the same bits.  One
 * workspace size serves both calls: scorp_pose_fit_workspace_bytes(n_pairs, n_hypotheses) (n_hypotheses 1 for the Adam
 * fit), 256-byte aligned.  The inputs are only read.
 *
 * scorp_pose_ransac: samples[n_hypotheses, 3] int32 are the pair indices of every hypothesis, drawn by the caller (the
 * library holds no random numbers).  Per hypothesis: Umeyama (method SCORP_POSE_UMEYAMA: cov = sum (p - pm)(q - qm)^T
 * = U S V^T, D = diag(1, 1, det(U V^T) < 0 ? -1 : 1), R = V D U^T, s = sum(S diag D) / sum |p - pm|^2, t = qm - s R pm) or
 * Kabsch (SCORP_POSE_KABSCH: the same with s = 1) on its three pairs, then the number of pairs with
 * |R (s p) + t - q| < threshold (strict) into out_counts[n_hypotheses].  The winner is the FIRST hypothesis with the
 * highest count; with min_inlier_ratio > 0 the first whose count exceeds min_inlier_ratio * n_pairs, if there is one.
 * out_winner[2] = {its index, its count}, out_inlier_mask[n_pairs] (0 / 1) its inliers, and out_R[3, 3] (row-major),
 * out_t[3], out_s[1] the same fit over those inliers.  A hypothesis run alone gets the count it gets in a batch.
 * Synchronises before it returns (reads a status word).  SCORP_ERR_INVALID: n_pairs < 3, n_hypotheses outside
 * [1, 65535], a sample index outside [0, n_pairs), threshold not finite, an unknown method, a NULL pointer, a workspace
 * too small or misaligned (none of these launches anything but the index check, which is the fit kernel's);
 * SCORP_ERR_NO_INLIERS: the winner has fewer than 3 inliers (the reference raises), out_R / out_t / out_s are not written.
 *
 * scorp_pose_adam_9dof: `iterations` steps of torch.optim.Adam (lr, betas 0.9 / 0.999, eps 1e-8) in ONE kernel launch on
 * t[3], q[4], qo[4], l[3] with M = R(q) Ro(qo)^T diag(s) Ro(qo), s = scale_min + (scale_max - scale_min) sigmoid(l),
 * R(q) = I + 2 B(q) / (q.q), and the loss
 *   mean |M p + t - q|^2 + lambda_reg_scale (mean (l - 1)^2 + mean (s - mean s)^2)
 *                        + lambda_reg_rot arccos(clamp((tr R - 1) / 2, -1, 1))^2,
 * gradients analytic, the data term through the float64 moments of the pairs about their centroids.  Start: t = 0.01,
 * q = (0.9, 0.01, 0.01, 0.01) (fp32-rounded, as the reference), qo = (1, 0, 0, 0), l = logit of init_scale[3] (a HOST
 * pointer) inside the bounds; an init_scale outside [scale_min, scale_max] becomes the mid-point for all three axes.
 * Where the rotation term has no finite derivative (|c| >= 1: R the identity or a half turn; the reference's autograd
 * gives NaN or an infinity there) its gradient is taken as 0.  out[25] = R (9, row-major), t (3), s (3), Ro (9), the loss
 * of the last step.  out_loss (may be NULL): the loss of steps loss_every, 2 loss_every, ... (as the reference prints
 * it, before that step's update), at most loss_capacity values.  Does not synchronise.  SCORP_ERR_INVALID: n_pairs < 3,
 * iterations outside [0, 1000000] (one wave runs them all: the bound keeps a call to seconds), non-finite
 * hyper-parameters, scale_max <= scale_min, loss_every < 1 with out_loss, a NULL pointer, a workspace too small or
 * misaligned. */
#define SCORP_POSE_UMEYAMA 0
#define SCORP_POSE_KABSCH 1
size_t scorp_pose_fit_workspace_bytes(int32_t n_pairs, int32_t n_hypotheses);
int scorp_pose_ransac(const double *source, const double *target, int32_t n_pairs, const int32_t *samples,
                      int32_t n_hypotheses, double threshold, double min_inlier_ratio, int32_t method, double *out_R,
                      double *out_t, double *out_s, int32_t *out_winner, int32_t *out_counts, uint8_t *out_inlier_mask,
                      void *workspace, size_t workspace_bytes, scorp_stream_t stream);
int scorp_pose_adam_9dof(const double *source, const double *target, int32_t n_pairs, int32_t iterations, double lr,
                         double lambda_reg_scale, double lambda_reg_rot, double scale_min, double scale_max,
                         const double *init_scale, double *out, double *out_loss, int32_t loss_every, int32_t loss_capacity,
                         void *workspace, size_t workspace_bytes, scorp_stream_t stream);

/* ---- multi-view TSDF fusion (gs2dgs/utils/mesh_utils.py:196-247 compute_sdf_perframe / compute_unbounded_tsdf) ----
 * Every sample runs over all views in ONE launch with its running state in registers.  All pointers are device pointers.
 * views:   depth[V, H, W], rgb[V, 3, H, W] (NULL: no colour), full_proj[V, 16] = each view's full_proj_transform as
 *          stored (row-vector convention: p_h = [x y z 1] @ M, M row-major); every view has the same resolution.
 * samples: the points xyz[*, 3], or (xyz NULL) the lattice x[nx], y[ny], z[nz] whose sample g = (ix ny + iy) nz + iz
 *          (C order, z fastest).  The call handles the samples g in [first, first + count) and writes out_tsdf[g] and
 *          out_rgb[3 g ..] - the arrays are addressed by the global index, so a caller splits a large M into calls by
 *          moving `first` alone.  count <= (2^31 - 1) 256.
 * params:  contracted != 0: the sample s lies in the contracted space, n = |s|, trunc = 5 voxel_size, times
 *          1 / (2 - min(n, 1.9)) where n > 1, and the world point is uncontract(s) radius + center (uncontract(y) = y for
 *          n < 1, y / n / (2 - n) otherwise); else trunc = 5 voxel_size and s is the world point.
 * Per sample: tsdf = 1, w = 1, rgb = 0; then for view i = 0 .. V-1 in order: p = [s 1] @ M_i, zc = p.w, pix = p.xy / p.w,
 * inside = all(pix > -1) & all(pix < 1) & zc > 0 (a NaN compares false), d = the bilinear sample of depth_i at pix
 * (align_corners, border padding; a corner of weight 0 past the last row / column is not read), sdf = d - zc, and where
 * inside & sdf > -trunc:  tsdf = (tsdf w + clamp(sdf / trunc, -1, 1)) / (w + 1), rgb likewise with the bilinear colour,
 * w += 1.  out_rgb may be NULL (then views->rgb is not read).  Does not synchronise.  SCORP_ERR_INVALID: a NULL pointer,
 * num_views < 1, width or height < 2, count < 1 (or above the bound, or past the lattice), voxel_size <= 0, radius <= 0
 * with contracted, out_rgb without views->rgb. */
typedef struct ScorpTsdfViews {
  const float *depth;
  const float *rgb;
  const float *full_proj;
  int32_t num_views, width, height, _pad;
} ScorpTsdfViews;
typedef struct ScorpTsdfSamples {
  const float *xyz;
  const float *x, *y, *z;
  int32_t nx, ny, nz, _pad;
  uint64_t first, count;
} ScorpTsdfSamples;
typedef struct ScorpTsdfParams {
  double voxel_size; /* trunc = (float)(5 voxel_size): the reference forms the product in double */
  float center[3];
  float radius;
  int32_t contracted, _pad;
} ScorpTsdfParams;
int scorp_tsdf_fuse(const ScorpTsdfViews *views, const ScorpTsdfSamples *samples, const ScorpTsdfParams *params,
                    float *out_tsdf, float *out_rgb, scorp_stream_t stream);

/* ---- surface extraction from a dense grid: naive surface nets, no tables ----
 * f[nx, ny, nz] fp32 in C order with the coordinate arrays x[nx], y[ny], z[nz]; a lattice point is INSIDE when
 * f < level.  Cell (i, j, k), 0 <= i < nx - 1 (likewise j, k), linear index (i (ny - 1) + j)(nz - 1) + k, is ACTIVE when
 * its 8 corners are neither all inside nor all outside.  An active cell owns one vertex: the mean over its sign-changing
 * edges (x-edges, then y-edges, then z-edges, each by ascending first corner, corner index = 4 di + 2 dj + dk) of the
 * crossing at t = (level - f0) / (f1 - f0), in the cell's own coordinates, then mapped through the coordinate arrays
 * (x[i] + frac (x[i + 1] - x[i])).  A lattice edge q -> q + e_a whose ends differ in inside-ness, with the other two
 * indices of q in 1 .. n - 2, gives the quad of the four cells round it, (b, c) = the axes after a in cyclic order:
 * c00 = cell(q), c10 = cell(q - e_b), c11 = cell(q - e_b - e_c), c01 = cell(q - e_c), as the triangles (c00, c10, c11),
 * (c00, c11, c01) when q is inside and reversed, (c00, c11, c10), (c00, c01, c11), otherwise: the normal points from
 * inside to outside.  Vertices follow the ascending cell index, quads the ascending linear index of q, then a: two
 * passes with a scan (the caller's) between them, no atomics.
 *   count_cells:   out_flags[cells] = 1 for an active cell, else 0
 *   emit_vertices: cell_scan[cells] = the INCLUSIVE int32 prefix sum of the flags; vertex cell_scan[c] - 1 of every active
 *                  cell c into out_vertices[num_vertices, 3]
 *   count_faces:   out_counts[nx ny nz] = quads of lattice point q (0 .. 3)
 *   emit_faces:    edge_scan[nx ny nz] = the inclusive int32 prefix sum of the counts; the two triangles of quad r into
 *                  out_faces[2 r .. 2 r + 1, 3] (int32 vertex indices), num_quads in all
 * None synchronises.  SCORP_ERR_INVALID: a NULL pointer, a dimension < 2, more than (2^31 - 1) 256 lattice points, more
 * than 2^31 - 1 vertices or quads. */
int scorp_isosurface_count_cells(const float *f, int32_t nx, int32_t ny, int32_t nz, float level, uint8_t *out_flags,
                                 scorp_stream_t stream);
int scorp_isosurface_emit_vertices(const float *f, const float *x, const float *y, const float *z, int32_t nx, int32_t ny,
                                   int32_t nz, float level, const int32_t *cell_scan, int64_t num_vertices,
                                   float *out_vertices, scorp_stream_t stream);
int scorp_isosurface_count_faces(const float *f, int32_t nx, int32_t ny, int32_t nz, float level, uint8_t *out_counts,
                                 scorp_stream_t stream);
int scorp_isosurface_emit_faces(const float *f, int32_t nx, int32_t ny, int32_t nz, float level, const int32_t *cell_scan,
                                const int32_t *edge_scan, int64_t num_quads, int32_t *out_faces, scorp_stream_t stream);

/* ---- marching cubes on a dense grid: one vertex per crossed lattice edge, triangles from a generated case table ----
 * Grid, coordinates, INSIDE (f < level) and corner numbering (n = 4 di + 2 dj + dk) as for scorp_isosurface_*.  The edges of a
 * cell are numbered 0 .. 11: the x-edges, then the y-edges, then the z-edges, each by ascending first corner (x: corners 0, 1,
 * 2, 3; y: 0, 1, 4, 5; z: 0, 2, 4, 6); edge e has the axis e / 4.  The CASE of a cell has bit n set when corner n is inside.
 *
 * Vertices.  A lattice edge q -> q + e_a (q_a + 1 < n_a) whose ends differ in inside-ness carries ONE vertex, shared by every
 * cell round it: along the axis c[q_a] + t (c[q_a + 1] - c[q_a]) with t = (level - f0) / (f1 - f0), f0 = f(q), f1 = f(q + e_a)
 * (fp32, no contraction), the other two coordinates straight from the coordinate arrays.  Vertices come in ascending (linear
 * index of q, axis).  A crossing exactly on a lattice point (f0 == level) gives coincident vertices and zero-area triangles;
 * they are kept.
 *
 * Triangles.  The table (csrc/mc_table.hpp, generated by scorp_amd/mc_table.py: 256 rows of 16 bytes = five triangles x three
 * edge ids, 0xFF padding, the count in the last byte) follows this rule.  Each of the six cube faces has 0, 2 or 4 crossed
 * edges; two crossings are joined; with four (two inside corners on a face diagonal) the two edges at each INSIDE corner are
 * joined, the inside corners being cut off separately.  The choice depends on the face's four signs alone, so the two cells
 * that share a face agree and the surface is closed.  Every crossed edge then has two partners; the loops are the cycles of
 * that graph, opened at the lowest unused edge id, oriented so that the Newell normal over the edge midpoints agrees with the
 * sum over the loop's edges of (outside end - inside end), and rotated to start at their lowest edge id.  A loop p[0 .. k - 1]
 * is triangulated by the first triangulation none of whose diagonals joins two crossings on one cube face, in this order:
 * tri(p) = the triangle (p[0], p[m], p[k - 1]) with the apex m descending from k - 2 to 1, for each apex every tri(p[0 .. m])
 * (outer) with every tri(p[m .. k - 1]) (inner), listed left part, apex triangle, right part - the fan from p[0] comes first.
 * The normals point from inside to outside.  The table is this project's own; it was compared with no other library's.
 * Triangles come in ascending cell index, then table order; the index of edge id e of cell c is the vertex of the lattice edge
 * (q, a) = (c + corner(n0(e)), e / 4):  edge_scan[q] - popc(mask[q]) + popc(mask[q] & ((1 << a) - 1)).
 *
 * Two passes with a scan (the caller's) between them, no atomics:
 *   count_edges:   out_masks[nx ny nz]: bit a set when the edge q -> q + e_a exists and is crossed; out_counts = its popcount
 *   emit_vertices: edge_scan[nx ny nz] = the INCLUSIVE int32 prefix sum of the counts; the vertices of q from
 *                  edge_scan[q] - popc(mask[q]) on into out_vertices[num_vertices, 3]
 *   count_faces:   out_counts[cells] = triangles of cell c (0 .. 5)
 *   emit_faces:    face_scan[cells] = the inclusive int32 prefix sum of those counts; the triangles of cell c from
 *                  face_scan[c] - count on into out_faces[num_faces, 3] (int32 vertex indices)
 * None synchronises.  SCORP_ERR_INVALID: a NULL pointer, a dimension < 2, more than (2^31 - 1) 256 lattice points, more
 * than 2^31 - 1 vertices or triangles. */
int scorp_marching_cubes_count_edges(const float *f, int32_t nx, int32_t ny, int32_t nz, float level, uint8_t *out_masks,
                                     uint8_t *out_counts, scorp_stream_t stream);
int scorp_marching_cubes_emit_vertices(const float *f, const float *x, const float *y, const float *z, int32_t nx, int32_t ny,
                                       int32_t nz, float level, const uint8_t *edge_masks, const int32_t *edge_scan,
                                       int64_t num_vertices, float *out_vertices, scorp_stream_t stream);
int scorp_marching_cubes_count_faces(const float *f, int32_t nx, int32_t ny, int32_t nz, float level, uint8_t *out_counts,
                                     scorp_stream_t stream);
int scorp_marching_cubes_emit_faces(const float *f, int32_t nx, int32_t ny, int32_t nz, float level, const uint8_t *edge_masks,
                                    const int32_t *edge_scan, const int32_t *face_scan, int64_t num_faces, int32_t *out_faces,
                                    scorp_stream_t stream);

/* ---- connected triangles of a mesh (Open3D's cluster_connected_triangles, as gs2dgs/utils/mesh_utils.py:30 calls it) ----
 * faces[num_faces, 3] int32 vertex indices, each in [0, 2^31 - 1].  Two triangles are ADJACENT when they share an edge, an
 * edge being the unordered pair of vertex INDICES: positions do not count, and two triangles that touch at one vertex are
 * not adjacent.  An edge may carry any number of triangles (surface nets give edges with 4).  A degenerate triangle
 * contributes its three edges like any other, (v, v) included; there is no special case.  A cluster is a connected
 * component of that adjacency.  Clusters are numbered in ascending order of the smallest triangle index they contain (the
 * order in which a search over the triangles in index order opens them); cluster_n_triangles[c] is the triangle count of
 * cluster c, cluster_area[c] the sum of its triangles' areas 0.5 |(v1 - v0) x (v2 - v0)|, in float64 from the float32 vertices.
 * Lock-free union-find over the triangles with the edges matched through an open-addressing hash table; a root is only
 * hooked under a smaller index, so the integer outputs do not depend on the execution order.  The caller owns every buffer
 * and the scan between the last two calls:
 *   link:  keys[num_slots] (uint64), owner[num_slots] (int32) and parent[num_faces] (int32) are scratch the call fills
 *          itself, the caller pre-fills nothing; num_slots is a power of two >= 6 num_faces (3 num_faces insertions: load
 *          <= 0.5) and <= 2^32.  A key is min(a, b) << 32 | max(a, b).
 *   roots: out_root[t] = the smallest triangle index of t's cluster, out_is_root[t] = (out_root[t] == t) as one byte.
 *   stats: root_scan[num_faces] = the INCLUSIVE int32 prefix sum of the bytes, num_clusters its last entry;
 *          out_cluster[t] = root_scan[root[t]] - 1, out_count[num_clusters] and - unless out_area or vertices is NULL -
 *          out_area[num_clusters] (float64), both zeroed by the call.  A vertex index outside [0, num_vertices) is not read
 *          and its triangle adds area 0.  The counts are exact.  The areas are float64 sums by atomic adds: they depend on
 *          the order of arrival in their last bits (within num_faces 2^-52 of the summed area), two calls need not agree there.
 * None synchronises.  SCORP_ERR_INVALID: a NULL pointer (other than out_area / vertices), num_faces < 1 or > 2^28,
 * num_slots not a power of two, < 6 num_faces or > 2^32, num_clusters outside [1, num_faces]. */
int scorp_mesh_cluster_link(const int32_t *faces, int64_t num_faces, uint64_t *keys, int32_t *owner, uint64_t num_slots,
                            int32_t *parent, scorp_stream_t stream);
int scorp_mesh_cluster_roots(const int32_t *parent, int64_t num_faces, int32_t *out_root, uint8_t *out_is_root,
                             scorp_stream_t stream);
int scorp_mesh_cluster_stats(const int32_t *faces, const float *vertices, int64_t num_vertices, const int32_t *root,
                             const int32_t *root_scan, int64_t num_faces, int64_t num_clusters, int32_t *out_cluster,
                             int32_t *out_count, double *out_area, scorp_stream_t stream);

/* ---- mesh simplification by vertex clustering (what Open3D's simplify_vertex_clustering does; the reference reduces its
 * meshes through Open3D and TRELLIS post-processing) ----
 * Open3D could not be run where this was written.  The rules below ARE the specification; nothing was compared with
 * Open3D's own output.  Edge-collapse decimation to a target triangle count is the next block (scorp_mesh_decimate_*).
 *
 * Inputs: vertices[Nv, 3] float32, finite; colors[Nv, 3] float32; faces[F, 3] int32 in [0, Nv); voxel_size h > 0 (a double);
 * the placement, average (quadric = 0) or quadric.  All arithmetic below is float64 from the float32 values, every product,
 * quotient and sum rounded on its own (no fp contraction), sums of three terms as (a + b) + c.
 *
 * 1. Cells.  min_bound[k] is the smallest coordinate k of all vertices (float32), origin[k] = double(min_bound[k]) - 0.5 h.
 *    Vertex v lies in cell i[k] = floor((double(v[k]) - origin[k]) / h): one subtraction and one division.  Membership is an
 *    exact integer function of the inputs; a vertex on a cell face belongs to the upper cell.  Every i[k] must be < 2^21
 *    (cell key = i[0] << 42 | i[1] << 21 | i[2], 63 bits).  Every vertex takes part, whether a face references it or not.
 * 2. Numbering.  Cells are numbered in ascending order of the smallest vertex index they contain; vertex_cell[v] is that
 *    number, C the cell count, output vertex c belongs to cell c.
 * 3. Colour and mean.  colour[c] and mean[c] are the sums of the members' colours / positions divided by the member count,
 *    then rounded to float32.  With the average placement mean[c] is the output position.
 * 4. Quadric placement.  p_c[k] = origin[k] + (i[k] + 0.5) h is the cell centre.  Every triangle (v0, v1, v2) with
 *    N = (v1 - v0) x (v2 - v0), |N| = sqrt((Nx^2 + Ny^2) + Nz^2) > 0 has area a = 0.5 |N| and unit normal n = N / |N|.  For each
 *    of its three corners, with that corner's cell c: d = -((nx (v0x - p_cx) + ny (v0y - p_cy)) + nz (v0z - p_cz)), then
 *    A_c[j][k] += (a n[j]) n[k] for j <= k (six entries; A_c is symmetric) and b_c[k] += (a d) n[k].  One contribution per
 *    corner: two corners in one cell add twice, there is no special case.  Zero-area triangles add nothing.
 *    m = (the float64 mean before its rounding) - p_c; sigma_1 >= sigma_2 >= sigma_3 and u_i the eigenpairs of A_c;
 *      x = m + sum over {i : sigma_i > 1e-3 sigma_1} of u_i (u_i . (-b_c - A_c m)) / sigma_i,
 *    formed as r[k] = -b_c[k] - ((A_c[k][0] m[0] + A_c[k][1] m[1]) + A_c[k][2] m[2]), t_i = ((u_i[0] r[0] + u_i[1] r[1]) +
 *    u_i[2] r[2]) / sigma_i, and x = m, then x += u_i t_i for i = 1, 2, 3 in turn.
 *    If sigma_1 = 0, or some |x[k]| > h (the point has left the cell by more than half a cell), the output position is
 *    mean[c] itself, bit for bit; otherwise it is float32(p_c + x).  A cell with ONE member keeps mean[c] as well, which is
 *    that vertex: every triangle that adds to the cell has the vertex as a corner, so it lies on all their planes and is
 *    the exact minimiser (r = 0); the solve would return it plus the rounding residue of r, some 1e-16 h, which is all there
 *    is of a coordinate whose exact value is 0.  A mesh whose vertices all have cells of their own comes back unchanged.  On a flat cell the point is the mean projected onto the
 *    plane, on a crease it slides to the crease, at a corner it lands on the corner.
 * 5. Faces.  Each face is mapped through vertex_cell; a face with two equal cells is dropped; the rest are rotated
 *    cyclically so that the smallest cell number comes first (the orientation stays).  Among faces that are then equal as
 *    ORDERED triples only the one with the smallest input index is kept: (a, b, c) and (a, c, b) are different faces.
 *    Survivors keep their input order.
 * The integer outputs (vertex_cell, C, the faces and their keep flags) do not depend on the execution order: both hash
 * tables resolve their slots by atomic min on an index.  Positions and colours come from float64 sums by atomic adds and
 * depend on the order of arrival in their last bits: two calls need not agree there (the float32 results agree within one
 * ulp wherever no decision of rule 4 sits on its threshold).
 *
 * The caller owns every buffer and the scans between the calls; scratch tables are filled by the call that uses them:
 *   cells:      keys[num_slots] (uint64) and owner[num_slots] (int32) are scratch, num_slots a power of two >= 2 num_vertices
 *               and <= 2^31; min_bound[3] is DEVICE memory (the stream stays asynchronous).  out_slot[v] = the slot of v's
 *               cell.  A condition on device data cannot fail the call without a synchronisation: out_overflow (one int32,
 *               device) is set to 0 by the call and to 1 when a cell index falls outside [0, 2^21) (or a coordinate is not
 *               finite); that vertex gets slot -1 and the outputs of the later calls are then meaningless (never out of
 *               bounds).  A caller that knows the bounds on the host checks the extent itself and reports SCORP_ERR_INVALID's
 *               meaning there, as scorp_amd/mesh/simplify.py does.
 *   roots:      out_rep[v] = the smallest vertex index of v's cell, out_is_root[v] = (out_rep[v] == v) as one byte.
 *   accumulate: rep_scan[num_vertices] = the INCLUSIVE int32 prefix sum of the bytes, num_cells its last entry.
 *               out_vertex_cell[v] = rep_scan[rep[v]] - 1; out_cell_ijk[num_cells, 3] (int32) the cells' indices;
 *               out_acc[num_cells, 16] (float64, zeroed by the call): position sums 3, colour sums 3, member count, A_c as
 *               xx xy xz yy yz zz, b_c 3 (the last nine stay 0 with quadric = 0, and faces may then be NULL).
 *   place:      out_vertices[num_cells, 3], out_colors[num_cells, 3] by rules 3 and 4.
 *   faces:      table[num_slots] (int32) is scratch, num_slots a power of two >= 2 num_faces and <= 2^31.
 *               out_faces[num_faces, 3] = the rotated triples ((-1, -1, -1) for a face with two equal cells),
 *               out_keep[num_faces] one byte per face; the caller scans the bytes and compacts.
 * None synchronises.  SCORP_ERR_INVALID: a NULL pointer, num_vertices < 1 or > 2^30, num_faces < 1 or > 2^28, voxel_size not
 * positive and finite, num_slots not a power of two, too small or > 2^31, num_cells outside [1, num_vertices]. */
int scorp_mesh_simplify_cells(const float *vertices, int64_t num_vertices, const float *min_bound, double voxel_size,
                              uint64_t *keys, int32_t *owner, uint64_t num_slots, int32_t *out_slot, int32_t *out_overflow,
                              scorp_stream_t stream);
int scorp_mesh_simplify_roots(const int32_t *owner, uint64_t num_slots, const int32_t *slot, int64_t num_vertices,
                              int32_t *out_rep, uint8_t *out_is_root, scorp_stream_t stream);
int scorp_mesh_simplify_accumulate(const float *vertices, const float *colors, int64_t num_vertices, const int32_t *faces,
                                   int64_t num_faces, const float *min_bound, double voxel_size, const int32_t *rep,
                                   const int32_t *rep_scan, int64_t num_cells, int32_t quadric, int32_t *out_vertex_cell,
                                   int32_t *out_cell_ijk, double *out_acc, scorp_stream_t stream);
int scorp_mesh_simplify_place(const double *acc, const int32_t *cell_ijk, int64_t num_cells, const float *min_bound,
                              double voxel_size, int32_t quadric, float *out_vertices, float *out_colors, scorp_stream_t stream);
int scorp_mesh_simplify_faces(const int32_t *faces, int64_t num_faces, const int32_t *vertex_cell, int64_t num_vertices,
                              int32_t *table, uint64_t num_slots, int32_t *out_faces, uint8_t *out_keep, scorp_stream_t stream);

/* ---- edge-collapse decimation to a target triangle count (what Open3D's simplify_quadric_decimation and the simplify
 * step of TRELLIS post-processing are used for) ----
 * Open3D could not be run where this was written.  The rules below ARE the specification; nothing was compared with
 * Open3D's own output.  tests/mesh_decimate_reference.py restates them in plain Python.
 *
 * Inputs: vertices[Nv, 3] float32, finite; colors[Nv, 3] float32; faces[F, 3] int32 in [0, Nv); the target triangle count
 * >= 0; maximum_error >= 0 (may be +inf); boundary_weight >= 0, finite.  All arithmetic is float64, every product,
 * quotient, sum and square root rounded on its own (no fp contraction), sums of three terms as (a + b) + c; u . w means
 * (u0 w0 + u1 w1) + u2 w2, |u|^2 = u . u, u x w = (u1 w2 - u2 w1, u2 w0 - u0 w2, u0 w1 - u1 w0).
 *
 *  0. State.  origin[k] = double(min over the vertices of coordinate k); P[v] = double(vertex v) - origin; the colour C[v]
 *     as doubles; the member count n[v] = 1.  Faces with two equal indices are dropped, the rest keep their order.  Every
 *     vertex has a quadric Q[v] = (A as xx xy xz yy yz zz, b[3], c), ten doubles.  Adding the plane (unit normal m, offset
 *     d) with weight w to a quadric means, with wm = (w m0, w m1, w m2) and wd = w d:  A_jk += wm_j m_k (j <= k),
 *     b_k += wd m_k, c += wd d.
 *  1. Initial quadrics, gathered per vertex, never scattered: Q[v] starts at 0 and v visits its faces in ascending face
 *     index.  A face (i0, i1, i2) with N = (P[i1] - P[i0]) x (P[i2] - P[i0]) and |N| = sqrt(N . N) > 0 adds the plane
 *     (n = N / |N|, d = -(n . P[i0])) with weight 0.5 |N|.  Then its edges k = 0, 1, 2, from corner k to corner k + 1 (mod 3),
 *     in that order: an edge (va, vb) that lies in exactly one face and has v as an end adds a second plane, with e =
 *     P[vb] - P[va], M = e x n, |M| = sqrt(M . M) > 0: (m = M / |M|, d = -(m . P[va])) with weight boundary_weight (e . e).
 *     Faces of zero area add nothing.
 *  2. Per round; `round` counts from 1, F is the current face count, K = F - target.  The loop ends when K <= 0 or a round
 *     has no candidate.  The edges are the unique pairs (lo < hi) of the current faces, numbered in ascending (lo, hi); each
 *     carries the count of its faces.  A vertex is BOUNDARY when it is on an edge with one face, LOCKED when it is on an edge
 *     with three or more.
 *  3. Candidates.  An edge is a candidate only if: it has 1 or 2 faces; neither end is locked; it is not a 2-face edge
 *     between two boundary vertices; the link condition holds - the set of common neighbours of lo and hi (u neighbours v
 *     when (u, v) is a current edge) equals the set of apexes of the edge's faces, and that set has as many members as the
 *     edge has faces; its cost (rule 4) is <= maximum_error; the flip test (rule 5) passes.
 *  4. Placement and cost.  Q = Q[lo] + Q[hi], element by element, lo's term first; A00 .. A22, b0 .. b2, c its parts.
 *       c00 = A11 A22 - A12 A12   c01 = A02 A12 - A01 A22   c02 = A01 A12 - A02 A11
 *       c11 = A00 A22 - A02 A02   c12 = A01 A02 - A00 A12   c22 = A00 A11 - A01 A01      (c10 = c01, c20 = c02, c21 = c12)
 *       det = (A00 c00 + A01 c01) + A02 c02,    x_k = -((c_k0 b0 + c_k1 b1) + c_k2 b2) / det,
 *     with mid = 0.5 (P[lo] + P[hi]) and t = (A00 + A11) + A22.  The solved point is taken iff det > 1e-9 ((t t) t) and
 *     |x - mid|^2 <= 4 |P[hi] - P[lo]|^2 (both false for NaN).  Otherwise x is whichever of P[lo], P[hi], mid has the
 *     least cost, ties in that order.
 *       cost(x) = max(0, ((s2 + 2 s1) + 2 s0) + c),   s2 = (A00 (x0 x0) + A11 (x1 x1)) + A22 (x2 x2),
 *       s1 = (A01 (x0 x1) + A02 (x0 x2)) + A12 (x1 x2),   s0 = (b0 x0 + b1 x1) + b2 x2.
 *     The two constants are conditions, not measurements: with them the yardstick takes the cube, the sphere and the sheets
 *     of tests/mesh_decimate_reference.py to their targets through the cofactor solve.
 *  5. Flip test.  For every current face (i0, i1, i2) that contains lo or hi but not both: N_old = (P[i1] - P[i0]) x
 *     (P[i2] - P[i0]), N_new the same with that end's position replaced by x; N_old . N_new > 0 is required.
 *  6. Window.  The candidates sorted by (cost, edge number) ascending; the first max(1, K div 2) are the window.
 *  7. Priority.  h(e) = mix((lo << 32 | hi) ^ mix(round)) >> 1, mix the splitmix64 finaliser modulo 2^64: z += 0x9E3779B97F4A7C15;
 *     z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31.  The window's edges are
 *     ranked by (h, edge number); the rank is an int32.  (Ranking by cost instead left two collapses per round on a cube.)
 *  8. Independent set.  vmin[v] = the least rank of a window edge at v, 2^31 - 1 if there is none; vmin2[v] = the least of
 *     vmin[v] and vmin[u] over all current edges (u, v).  A window edge is SELECTED iff rank == vmin2[lo] == vmin2[hi].
 *     No vertex of a selected edge equals or neighbours a vertex of another selected edge:  let e (rank r) and e' (rank r')
 *     be selected and w a vertex of e' that equals or neighbours the vertex v of e.  vmin[w] <= r' since e' is at w, and
 *     vmin2[v] <= vmin[w], so r = vmin2[v] <= r'.  By the same argument with the roles exchanged r' <= r; ranks are
 *     distinct, so e = e'.  Hence every test of rules 3 - 5 read only data that no other collapse of the round changes.
 *  9. Budget.  Walk the selected edges in rank order with the running sum of their face counts; an edge is applied iff the
 *     sum before it is < K.  For any reachable target target - 1 <= F_out <= target.  The window's rank-0 edge is always
 *     selected and applied, so a round with a candidate removes a face and the loop ends within F rounds.
 * 10. Apply.  P[lo] = x; Q[lo] = Q[lo] + Q[hi]; C[lo] = (n_lo C[lo] + n_hi C[hi]) / (n_lo + n_hi) per channel, the counts as
 *     doubles; n[lo] += n[hi]; faces are mapped through hi -> lo and those with two equal indices are dropped, the
 *     survivors keep their order.
 * 11. Output.  Vertices no face references are dropped, the survivors keep their order and the faces are re-indexed;
 *     positions are float32(origin + P), colours float32(C).
 * No float is summed by atomics: every result, float or integer, is a function of the input alone, and two runs agree
 * bit for bit.
 *
 * The caller owns every buffer and, between the calls, the sorts, the scans, the compaction and ONE `unique` per round over
 * the 3 F keys lo << 32 | hi of the faces' edges (edge k of face t at 3 t + k), which yields edge_keys[E] (int64, ascending:
 * the edge numbering), face_edge[F, 3] (int32) and edge_faces[E] (int32 counts).  vf_start[Nv + 1], vf_face[3 F] (int32) is
 * the vertex -> face CSR of the current faces, every vertex's faces in ascending index.  The state is positions[Nv, 3],
 * quadrics[Nv, 10], colors[Nv, 3] (float64) and count[Nv] (int32); Nv never changes, a collapsed vertex just loses its faces.
 *   quadrics:   rule 1, once, from the cleaned faces of rule 0.
 *   flags:      out_flags[Nv] (int32, zeroed by the call): bit 0 boundary, bit 1 locked.
 *   candidates: out_cost[E] = the cost of rule 4, or +inf for an edge that is no candidate; out_x[E, 3] its point.
 *   hash:       out_hash[i] = h(window[i]) (int64, < 2^63) for the window's edge numbers window[W]; the caller passes them in
 *               ascending edge number and sorts stably by the hash, which ranks by (h, edge number).
 *   select:     ranked[W] = the window's edges by rank; vmin[Nv], vmin2[Nv] (int32) are scratch the call fills;
 *               out_selected[W] one byte per rank.
 *   apply:      applied[W] one byte per rank (rule 9, the caller's prefix sum); rule 10 on the state; out_vmap[Nv] = the
 *               identity but for vmap[hi] = lo of the applied edges.
 *   faces:      out_faces[F, 3] = the faces through vmap, out_keep[F] = 0 for a face with two equal indices.
 * None synchronises.  An index that is out of range in a caller's array is never followed out of bounds.
 * SCORP_ERR_INVALID: a NULL pointer, num_vertices < 1 or > 2^30, num_faces < 1 or > 2^28, num_edges < 1 or > 3 num_faces,
 * num_window outside [1, num_edges], round < 1, maximum_error negative or NaN, boundary_weight negative or not finite. */
int scorp_mesh_decimate_quadrics(const double *positions, int64_t num_vertices, const int32_t *faces, int64_t num_faces,
                                 const int32_t *face_edge, const int32_t *edge_faces, int64_t num_edges, const int32_t *vf_start,
                                 const int32_t *vf_face, double boundary_weight, double *out_quadrics, scorp_stream_t stream);
int scorp_mesh_decimate_flags(const int64_t *edge_keys, const int32_t *edge_faces, int64_t num_edges, int64_t num_vertices,
                              int32_t *out_flags, scorp_stream_t stream);
int scorp_mesh_decimate_candidates(const double *positions, const double *quadrics, int64_t num_vertices, const int32_t *faces,
                                   int64_t num_faces, const int64_t *edge_keys, const int32_t *edge_faces, int64_t num_edges,
                                   const int32_t *vf_start, const int32_t *vf_face, const int32_t *flags, double maximum_error,
                                   double *out_cost, double *out_x, scorp_stream_t stream);
int scorp_mesh_decimate_hash(const int64_t *edge_keys, int64_t num_edges, const int32_t *window, int64_t num_window, int64_t round,
                             int64_t *out_hash, scorp_stream_t stream);
int scorp_mesh_decimate_select(const int64_t *edge_keys, int64_t num_edges, const int32_t *ranked, int64_t num_window,
                               int64_t num_vertices, int32_t *vmin, int32_t *vmin2, uint8_t *out_selected, scorp_stream_t stream);
int scorp_mesh_decimate_apply(const int64_t *edge_keys, int64_t num_edges, const int32_t *ranked, const uint8_t *applied,
                              int64_t num_window, const double *x, int64_t num_vertices, double *positions, double *quadrics,
                              double *colors, int32_t *count, int32_t *out_vmap, scorp_stream_t stream);
int scorp_mesh_decimate_faces(const int32_t *faces, int64_t num_faces, const int32_t *vmap, int64_t num_vertices, int32_t *out_faces,
                              uint8_t *out_keep, scorp_stream_t stream);

/* ---- measuring a mesh: exact point-to-mesh distance, surface sampling, nearest point of a cloud (what Open3D's
 * RaycastingScene.compute_closest_points, sample_points_uniformly and compute_point_cloud_distance are used for) ----
 * tests/mesh_distance_reference.py restates the distance by brute force in another formulation (project to the plane, else
 * the three segments) and the sampler from the same prefix array.
 *
 * Inputs: vertices[Nv, 3] float32, finite; faces[F, 3] int32 in [0, Nv); queries[Q, 3] float32; max_distance >= 0 (may be
 * +inf).  All arithmetic below is float64 on the float32 values, every product, quotient and sum rounded on its own (no fp
 * contraction), u . w = (u0 w0 + u1 w1) + u2 w2, u x w as in the decimation block.
 *
 *  1. Grid.  The grid of the ICP search (icp_search.hpp) over the bounding box of ALL vertices: centre ct, origin lo,
 *     cell edge h from the density 8 F (about one triangle per cell of a closed surface), at most min(8 F + 64, 2^30) cells
 *     and 1024 per axis.  Cell i of an axis is [lo + i h, lo + (i + 1) h]; every coordinate below is relative to ct.
 *  2. Registration.  A triangle is registered in every cell its bounding box overlaps: per axis the cells
 *     floor((min - lo) / h - 1e-9) .. floor((max - lo) / h + 1e-9), clamped to the grid.  The pad of 1e-9 cells is far above
 *     the rounding of that quotient (values <= 1024, so 2e-13) and of the bound of rule 6, so a cell the triangle touches is
 *     never dropped.  The (cell, triangle) pairs are a CSR in raster cell order (x fastest) built by count, exclusive scan
 *     and fill; the order inside a cell is not defined and nothing depends on it.
 *  3. Pair cap.  cap = 8 F + 4096.  The pairs are first only counted; while the count exceeds the cap, h *= 1.25, the cell
 *     counts per axis are taken again (lo and ct stay) and the count is repeated.  A one-cell grid has F pairs, so the loop
 *     ends; the 65th step forces one cell.  Memory is therefore bounded by F alone, whatever the triangles' sizes.
 *  4. Closest point on a triangle (A, B, C) to P, with the edges ab = B - A, ac = C - A, bc = C - B taken from the float32
 *     values themselves and ap = P - A from the centre-relative ones; n = ab x ac.  With d1 = ab . ap, d2 = ac . ap,
 *     bp = ap - ab, d3 = ab . bp, d4 = ac . bp, cp = ap - ac, d5 = ab . cp, d6 = ac . cp, in this order:
 *       d1 <= 0 and d2 <= 0: A.     d3 >= 0 and d4 <= d3: A + ab.
 *       vc = d1 d4 - d3 d2 <= 0, d1 >= 0, d3 <= 0: A + (d1 / (d1 - d3)) ab.
 *       d6 >= 0 and d5 <= d6: A + ac.
 *       vb = d5 d2 - d1 d6 <= 0, d2 >= 0, d6 <= 0: A + (d2 / (d2 - d6)) ac.
 *       va = d3 d6 - d5 d4 <= 0, d4 - d3 >= 0, d5 - d6 >= 0: (A + ab) + ((d4 - d3) / ((d4 - d3) + (d5 - d6))) bc.
 *       else the face: P - ((n . ap) / (n . n)) n.   (The offset along the normal, not a barycentric sum: on a sliver of
 *       aspect 1e6 the barycentric weights carry errors of 1e-5, the normal of 1e-10.)
 *     d^2 = |P - closest|^2.
 *  5. Degenerate faces.  n = (0, 0, 0) exactly: the closest of the closest points of the segments (A, B), (B, C), (C, A),
 *     ties in that order.  On a segment from a with e = b - a: t = (p - a) . e; a if not t > 0; a + e if t >= e . e; else
 *     a + (t / (e . e)) e.  Nothing is divided by an area.
 *  6. Walk.  Per query: a miss if a coordinate is not finite, or if the squared distance to the vertices' bounding box
 *     exceeds max_distance^2.  Else rings of cells at Chebyshev distance k = 0, 1, ... around the query's cell (clamped to
 *     one cell outside the grid): icp_ring_walk (icp_search.hpp) in float64.  After ring k everything outside its box is at
 *     least lb away, lb the least distance to the box's sides that are still inside the grid, computed in float64 from
 *     lo + i h; the walk ends when lb^2 > best or no side is left.  best starts at max_distance^2.  (lb alone is not held
 *     to "no contraction": lo + i h may be one fused multiply-add.  It decides where the walk ends, never a value, and the
 *     pad of rule 2 is far above either rounding.)
 *  7. Result.  The minimum over the triangles met of (d^2, face index) in lexicographic order, a hit iff d^2 <=
 *     max_distance^2: out_squared_distance = d^2, out_face, out_closest = float32(closest + ct).  A miss gives +inf, -1 and
 *     NaNs.  The value of a (query, triangle) pair depends on nothing but the pair and ct, so the result is a function of
 *     the inputs alone: not of the queries' order or number (ct and the grid come from the mesh only), of the launch shape,
 *     of the pairs' order, or of how often a triangle is met.
 *
 * build fills the workspace (scorp_mesh_distance_workspace_bytes(F, Q), 256-byte aligned) and SYNCHRONISES the stream (the
 * read-backs of rule 3); out_header, a host array of 8 int64 or NULL, receives the pair count, the cap, the cell count, the
 * cell cap, the three cell counts per axis and the number of growth steps.  query sorts the queries by the 30-bit Morton
 * code of the ICP source and runs rules 4 - 7 against a built workspace; num_faces = 0 (an empty mesh: all misses, no
 * workspace needed) and num_queries = 0 are allowed.  An index that is out of range is never followed.
 *
 * Sampler: sample i of n draws t = ((i + u(i, 0)) / n) A_total, A_total = area_prefix[F - 1], and takes the first face f
 * with area_prefix[f] > t (t = the float64 below A_total if rounding reached it), so a face of zero area is never taken;
 * area_prefix[F] is the caller's inclusive float64 prefix sum of the triangle areas.  u(i, k) = (mix(mix(mix(seed) ^ i) ^ k)
 * >> 11) 2^-53, mix the splitmix64 finaliser of decimation rule 7.  With s = sqrt(u(i, 1)), r = u(i, 2): w = (1 - s,
 * s (1 - r), s r) and the point is (w0 A + w1 B) + w2 C per coordinate, rounded once to float32.
 *
 * Nearest point: the grid search of the ICP (fp32 d^2 on centre-relative coordinates, ties to the lower original index,
 * searched to max_distance^2 (1 + 1e-5)), then the pair's d^2 in float64; a hit iff that is <= max_distance^2, else -1, +inf.
 *
 * SCORP_ERR_INVALID: a NULL pointer, num_vertices outside [1, 2^30], num_faces outside [1, 2^28] (query: [0, 2^28]),
 * num_queries / num_samples outside [0, 2^31 - 1], num_cloud outside [1, 2^30], max_distance negative or NaN, a workspace
 * that is too small or misaligned. */
size_t scorp_mesh_distance_workspace_bytes(int64_t num_faces, int64_t num_queries);
int scorp_mesh_distance_build(const float *vertices, int64_t num_vertices, const int32_t *faces, int64_t num_faces, void *workspace,
                              size_t workspace_bytes, int64_t *out_header, scorp_stream_t stream);
int scorp_mesh_distance_query(const float *vertices, int64_t num_vertices, const int32_t *faces, int64_t num_faces,
                              const float *queries, int64_t num_queries, double max_distance, double *out_squared_distance,
                              int32_t *out_face, float *out_closest, void *workspace, size_t workspace_bytes, scorp_stream_t stream);
int scorp_mesh_sample_points(const float *vertices, int64_t num_vertices, const int32_t *faces, int64_t num_faces,
                             const double *area_prefix, int64_t num_samples, uint64_t seed, float *out_points, int32_t *out_faces,
                             float *out_barycentric, scorp_stream_t stream);
size_t scorp_nearest_point_workspace_bytes(int32_t num_points, int32_t num_cloud);
int scorp_nearest_point_distance(const float *points, int32_t num_points, const float *cloud, int32_t num_cloud, double max_distance,
                                 double *out_squared_distance, int32_t *out_index, void *workspace, size_t workspace_bytes,
                                 scorp_stream_t stream);

/* ---- looking at a mesh: depth, face, barycentric and colour maps of a triangle mesh from any number of cameras, and the
 * number of views in which each face owns a pixel (a z-buffer rasterizer; scorp_amd/mesh/render.py) ----
 * The rules below ARE the specification, and three of them are this project's own: positions are snapped to 1/256 pixel,
 * nothing is clipped against the near plane (a triangle with a vertex behind it is dropped whole), and of two faces with
 * the same fp32 depth at a pixel the lower index wins.  Nothing was compared with Open3D's or any other renderer's output.
 * tests/mesh_render_reference.py restates coverage and depth with exact integers and fractions.
 *
 * Inputs (device): vertices[Nv, 3] float32; faces[F, 3] int32; colors[Nv, 3] float32 or NULL; full_proj[V, 16] float32, each
 * camera's full_proj_transform as stored (row-major m[r][c], a point is a ROW vector: the layout scorp_tsdf_fuse takes);
 * height H, width W; near > 0; flags; optionally support_depth[V, H, W] float32 with support_tolerance.
 *
 *  1. Projection, float64 on the float32 values, every product, quotient and sum rounded on its own (no fp contraction).
 *     For vertex (x, y, z): p_j = ((z m[2][j] + (y m[1][j] + x m[0][j])) + m[3][j]) for j = 0, 1, 3; w = p_3 (for this
 *     projection the view-space z), inv_w = 1.0 / w, sx = ((p_0 inv_w + 1) W - 1) 0.5, sy = ((p_1 inv_w + 1) H - 1) 0.5:
 *     the splat rasterizers' pixel convention, pixel (i, j) has its centre AT (i, j), so the maps line up with render_depth
 *     pixel for pixel.
 *  2. Snapping.  X = (int64) floor(sx 256 + 0.5), Y likewise: positions in units of 1/256 pixel.  A vertex is unusable for
 *     a view unless w > near, w < +inf, |floor(sx 256 + 0.5)| <= 2^29 and the same for y (a NaN fails every test).  A
 *     triangle with an unusable vertex is DROPPED for that view: there is no clipping against the near plane, so a triangle
 *     that crosses it disappears whole.  A face with an index outside [0, Nv) is dropped too; such an index is never followed.
 *  3. Set-up, all int64.  The edge function of the edge a -> b at P is E(P) = (b_Y - a_Y)(P_X - a_X) - (b_X - a_X)(P_Y - a_Y).
 *     With the corners (v_0, v_1, v_2), E_0 belongs to v_1 -> v_2, E_1 to v_2 -> v_0, E_2 to v_0 -> v_1 (the edge opposite
 *     corner k), and A = E_2(v_2) is twice the signed area: A > 0 for corners that run counter-clockwise as the image is
 *     looked at (x to the right, y down), the side of a face whose right-hand normal points at the camera.  A = 0: dropped.
 *     A < 0: dropped when SCORP_MESH_RENDER_CULL_BACKFACES is set, else corners 1 and 2 change places (local order
 *     v_0, v_2, v_1), which makes A > 0; rule 6 undoes the exchange.  E_0 + E_1 + E_2 = A at every P.  Coordinates are at
 *     most 2^29 in size and pixel centres at most 2^22, so a difference stays below 2^30 + 2^22, a product below 2^61 and an
 *     edge function below 2^62: nothing overflows.
 *  4. Coverage, exact.  The pixel centre P = (256 i, 256 j) belongs to the triangle iff for every k: E_k(P) > 0, or
 *     E_k(P) = 0 and the edge a -> b of E_k is a LEFT edge, b_Y - a_Y > 0 (it runs down the image), or a TOP edge,
 *     b_Y - a_Y = 0 and b_X - a_X < 0.  That is the sign of E_k at P + (eps, eps^2) for a vanishing eps > 0, so any set
 *     of triangles that tile a region without overlap own each pixel centre of it exactly once, on shared edges and at
 *     shared corners too.  Only centres with 0 <= i < W and 0 <= j < H inside the triangle's bounding box are looked at.
 *  5. Depth.  q = ((double) E_0 inv_w_0 + (double) E_1 inv_w_1) + (double) E_2 inv_w_2 in the local order, float64, no
 *     contraction; depth = (float) ((double) A / q), the perspective-correct view-space depth (> 0).  The z-buffer holds
 *     one uint64 per (view, pixel), cleared to all ones and updated by an unsigned 64-bit atomic minimum with the key
 *     (uint64) bits(depth) << 32 | face: the nearest depth wins, equal fp32 depths go to the lower face index.  The
 *     minimum is order-free, so the maps do not depend on the launch shape, on which path a triangle took, on the order
 *     the faces arrive in or on how many views share a call.
 *  6. Resolve, per (view, pixel).  An all-ones key: depth 0, face -1, barycentrics and colour 0.  Else depth and face from
 *     the key, and from the winner's set-up b_k = ((double) E_k inv_w_k) / q in the local order, put back into the face's
 *     own order (b_1 and b_2 change places when rule 3 exchanged the corners): out_barycentric[V, 3, H, W] = (float) b_k;
 *     out_color[V, 3, H, W] = (float) ((b_0 c_0 + b_1 c_1) + b_2 c_2) per channel, c_k the colour of the face's k-th
 *     vertex, float64 and rounded once.
 *  7. Visibility.  out_visible_views[F] int32 is INCREASED by the number of views of this call in which the face owns at
 *     least one pixel (the caller zeroes it; calls over chunks of the views accumulate).  With support_depth, a pixel
 *     counts only if support_depth > 0 there and fabsf(depth - support_depth) <= support_tolerance in fp32.  (A flag per
 *     (view, face) that any number of threads set to 1, then summed per face: order-free.)
 *
 * A triangle whose clipped box holds at most 64 pixel centres is walked by one thread, any other by a workgroup; the list
 * of the latter has room for every face of every view, so it cannot overflow and the call never reads anything back: it
 * does not synchronise.  Workspace: scorp_mesh_render_workspace_bytes (16 V Nv + 8 V H W + 5 V F bytes and padding; 0 for
 * sizes outside the limits), 256-byte aligned; after the call its first V uint32 hold the length of each view's list of
 * workgroup-walked triangles (a figure for measurements; no result depends on it).  out_barycentric, out_color and out_visible_views may be NULL and are then
 * skipped; num_faces = 0 renders empty maps.
 * SCORP_ERR_INVALID: a NULL required pointer (out_color without colors included), num_vertices outside [1, 2^30],
 * num_faces outside [0, 2^28], num_views outside [1, 65535], height or width outside [1, 16384], near not positive and
 * finite, unknown flags, support_tolerance negative or NaN beside a support_depth, a workspace too small or misaligned. */
#define SCORP_MESH_RENDER_CULL_BACKFACES 1u   /* rule 3: drop the faces with A < 0 */
size_t scorp_mesh_render_workspace_bytes(int64_t num_vertices, int64_t num_faces, int32_t num_views, int32_t height, int32_t width);
int scorp_mesh_render(const float *vertices, int64_t num_vertices, const int32_t *faces, int64_t num_faces, const float *colors,
                      const float *full_proj, int32_t num_views, int32_t height, int32_t width, double near, uint32_t flags,
                      const float *support_depth, float support_tolerance, float *out_depth, int32_t *out_face,
                      float *out_barycentric, float *out_color, int32_t *out_visible_views, void *workspace,
                      size_t workspace_bytes, scorp_stream_t stream);

/* ---- smoothing a mesh, and its normals: face and vertex normals, Laplacian and Taubin half-steps, the normal map of a
 * rendered mesh (what Open3D's compute_triangle_normals / compute_vertex_normals / filter_smooth_laplacian /
 * filter_smooth_taubin are used for; scorp_amd/mesh/smooth.py) ----
 * The rules below ARE the specification and they are this project's own.  Nothing here was or can be compared with Open3D's
 * output: Open3D was not available, and its summation order is not part of its interface.  The inverse-distance weights of
 * rule 7 are what Open3D's Laplacian filter is BELIEVED to use; that was not checked.  tests/mesh_smooth_reference.py
 * restates the rules as per-vertex loops over Python sets, lists and floats.
 *
 * Inputs (device): vertices[Nv, 3] float32; faces[F, 3] int32.  All arithmetic is float64 on the float32 values, every
 * product, quotient, square root and sum rounded on its own (no fp contraction), and each output is rounded to float32 once.
 *
 *  1. Sides.  A face (a, b, c) has the sides (a, b), (b, c), (c, a).  A side with equal ends is ignored.  Indices out of
 *     range are refused by the Python layer (check_mesh); the kernels skip them and never follow one.
 *  2. Neighbours of vertex v: the distinct other ends of the sides that name v, in ascending order, each once - however many
 *     faces share the side, so duplicate faces and non-manifold edges change nothing.  As a CSR: neighbor_offsets[Nv + 1]
 *     int32, neighbors[neighbor_offsets[Nv]] int32.
 *  3. Incident corners of v: one entry per face corner that names v, exactly 3 F entries in all, in ascending face index; a
 *     face that names v twice is listed twice.  As a CSR: corner_offsets[Nv + 1] int32, corner_faces[3 F] int32.
 *  4. Boundary.  A vertex is a boundary vertex when it is an end of an undirected side {a, b} that occurs exactly once over
 *     all faces.
 *  5. Face normal.  e1 = b - a, e2 = c - a; n = e1 x e2 component by component, n_x = e1_y e2_z - e1_z e2_y,
 *     n_y = e1_z e2_x - e1_x e2_z, n_z = e1_x e2_y - e1_y e2_x.  Its unit form is n / sqrt((n_x^2 + n_y^2) + n_z^2); a zero
 *     length gives (+0, +0, +0).
 *  6. Vertex normal: the float64 sum over the incident corners in rule 3's order, s = s + n per component, of n
 *     (SCORP_MESH_NORMALS_AREA: weighted by twice the face's area) or of n's unit form (SCORP_MESH_NORMALS_UNIFORM); the sum
 *     is normalised as in rule 5 and rounded to float32 once.  A zero sum and a vertex with no face give +0.  There is no
 *     angle weighting: it needs acos, which no reference here reproduces bit for bit.
 *  7. Half-step with factor f.  A vertex with no neighbour, and a fixed vertex, is copied.  Otherwise with p the vertex and
 *     q_j its neighbours in rule 2's order: s = s + w_j q_j per component and W = W + w_j, from s = 0 and W = 0; the new
 *     position is (float) (p + f (s / W - p)) per component.  SCORP_MESH_SMOOTH_UNIFORM: w_j = 1.
 *     SCORP_MESH_SMOOTH_INVERSE_DISTANCE: w_j = 1 / (sqrt((d_x^2 + d_y^2) + d_z^2) + 1e-12) with d = p - q_j.  Every
 *     half-step reads the float32 output of the half-step before it and writes another buffer (Jacobi, never in place).
 *  8. Filters (Python).  filter_smooth_laplacian(n, lambda) is n half-steps with factor lambda; filter_smooth_taubin(n,
 *     lambda, mu) is n times [lambda, mu]; the defaults are n = 1, lambda = 0.5, mu = -0.53.  n = 0 returns the input's
 *     positions bit for bit.  Faces and colours are never touched.  fix_boundary fixes rule 4's vertices.
 *
 * scorp_mesh_face_normals: out_normals[F, 3] = (float) n, or n's unit form when `normalized` is not 0; a face with an
 * index outside [0, Nv) gives +0.
 * scorp_mesh_vertex_normals: out_normals[Nv, 3] by rule 6.  A slice of the CSR is clamped to [0, 3 F] and an entry outside
 * [0, F) is skipped.
 * scorp_mesh_smooth: enqueues all num_steps half-steps, step k with factors[k] (HOST doubles, read before the call
 * returns), without synchronising.  It ping-pongs between `scratch` and `out` (each [Nv, 3] float32, neither may be
 * `vertices`; scratch may be NULL for num_steps <= 1) and the last half-step lands in `out` for odd and even counts alike;
 * num_steps = 0 copies vertices to out.  `fixed`: uint8[Nv], not 0 = the vertex is copied, or NULL.  A slice of the CSR is
 * clamped to [0, offsets[Nv]] and a neighbour outside [0, Nv) is skipped; a vertex whose neighbours are all skipped is copied.
 * scorp_mesh_normal_map: per (view, pixel) of a mesh render's face map[V, H, W] int32 and barycentric map[V, 3, H, W]
 * (rule 6 of the mesh-render block): out_normals[V, 3, H, W] float32 in world space.  With vertex_normals[Nv, 3] float32 the
 * value is ((b_0 N_a + b_1 N_b) + b_2 N_c) per component, normalised as in rule 5; with NULL it is the face's unit normal
 * of rule 5 and barycentric may be NULL.  A pixel whose face is -1, or outside [0, F), gives +0.
 * SCORP_ERR_INVALID: a NULL required pointer, num_vertices outside [1, 2^30], num_faces outside [0, 2^28], an unknown
 * weighting or weights, num_steps outside [0, 2^20], a factor that is not finite, aliased buffers, num_views outside
 * [1, 65535], height or width outside [1, 16384], vertex_normals without barycentric. */
#define SCORP_MESH_NORMALS_AREA 0
#define SCORP_MESH_NORMALS_UNIFORM 1
#define SCORP_MESH_SMOOTH_UNIFORM 0
#define SCORP_MESH_SMOOTH_INVERSE_DISTANCE 1
int scorp_mesh_face_normals(const float *vertices, int64_t num_vertices, const int32_t *faces, int64_t num_faces, int32_t normalized,
                            float *out_normals, scorp_stream_t stream);
int scorp_mesh_vertex_normals(const float *vertices, int64_t num_vertices, const int32_t *faces, int64_t num_faces,
                              const int32_t *corner_offsets, const int32_t *corner_faces, int32_t weighting, float *out_normals,
                              scorp_stream_t stream);
int scorp_mesh_smooth(const float *vertices, int64_t num_vertices, const int32_t *offsets, const int32_t *neighbors,
                      const uint8_t *fixed, const double *factors, int32_t num_steps, int32_t weights, float *scratch, float *out,
                      scorp_stream_t stream);
int scorp_mesh_normal_map(const float *vertices, int64_t num_vertices, const int32_t *faces, int64_t num_faces,
                          const float *vertex_normals, const int32_t *face_map, const float *barycentric, int32_t num_views,
                          int32_t height, int32_t width, float *out_normals, scorp_stream_t stream);

/* ---- bounded TSDF volume: sparse 16^3-voxel blocks, fused and meshed (the route of gs2dgs/utils/mesh_utils.py:138-180
 * extract_mesh_bounded, which hands the work to Open3D's ScalableTSDFVolume) ----
 * Open3D's volume could be neither read nor run where this was written.  The rules below ARE the specification; nothing
 * was compared with Open3D's own output.  All quantities are fp32 unless said otherwise, every product and sum rounded on
 * its own (no fp contraction), sums of three terms as (a + b) + c.
 *
 * Geometry.  A voxel has integer coordinates g = (gx, gy, gz); its sample point is its centre, voxel_length (g + 0.5).  A
 * block is 16^3 voxels: b = floor(g / 16) per axis (negative coordinates included), local index l = g - 16 b, linear index
 * (lx 16 + ly) 16 + lz.  Block key = (bx + 2^20) << 42 | (by + 2^20) << 21 | (bz + 2^20), each component in [-2^20, 2^20).
 * Ascending key order is the lexicographic order of (bx, by, bz); it is the block order of every output.
 *
 * Views.  depth[V, H, W] (0 = no measurement), rgb[V, H, W, 3] uint8 (optional), cam[V, 16] = the world-to-camera matrix
 * E[3, 4] row-major (p_cam = R p_w + t) followed by the pinhole fx, fy, cx, cy.  All views share one resolution.
 *
 * Touch (which blocks exist, and which views may write to them).  For view i, every pixel (u, v) with u % stride == 0,
 * v % stride == 0 and d = depth_i[v, u] > 0:  p_cam = ((u - cx) d / fx, (v - cy) d / fy, d),  p_w = R^T (p_cam - t);  every
 * block that meets the box [p_w - sdf_trunc, p_w + sdf_trunc] - per axis floor((p_w -+ sdf_trunc) / (16 voxel_length)) -
 * exists and carries bit i of its view mask (word i / 32, bit i % 32).  sdf_trunc <= 16 voxel_length is required, so at
 * most 27 blocks per pixel.
 *
 * Integrate.  Every voxel starts with tsdf = 0, w = 0, colour = 0.  Views run in order; view i skips a block whose mask
 * lacks bit i.  For the rest:  p = E [centre 1], skip unless p.z > 0;  u_f = p.x fx / p.z + cx + 0.5, v_f likewise;  skip
 * unless 1e-4 <= u_f < W - 1e-4 and 1e-4 <= v_f < H - 1e-4;  u = (int)u_f, v = (int)v_f (the nearest pixel, no
 * interpolation);  d = depth_i[v, u], skip unless d > 0;  sdf = (d - p.z) sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1);
 * where sdf > -sdf_trunc:  tsdf = (tsdf w + min(1, sdf / sdf_trunc)) / (w + 1),  colour = (colour w + rgb_i[v, u]) / (w + 1)
 * per channel in [0, 255],  w += 1.
 *
 * Surface (surface nets over the voxel centres: the rules of scorp_isosurface_* applied through block borders, level 0,
 * inside = tsdf < 0).  Cell g has the corners g + {0, 1}^3 and belongs to the block of g.  It is VALID when all eight
 * corners lie in existing blocks and have w > 0, ACTIVE when it is valid and its corners are neither all inside nor all
 * outside.  An active cell owns one vertex: the mean of its edge crossings, in the edge order of scorp_isosurface_*, at
 * voxel_length ((g + 0.5) + frac); its colour is the mean over the same edges of the linearly interpolated voxel colours
 * c0 + t (c1 - c0), divided by 255.  A lattice edge q -> q + e_a whose ends differ in inside-ness and whose four
 * surrounding cells are all valid gives the quad of those cells, diagonal and winding as in scorp_isosurface_* (the normal
 * points from inside to outside); it belongs to the block of q.  Vertices come in ascending (block rank, local cell index),
 * quads in ascending (block rank, local index of q, axis).  No atomic decides a position; the scans are the caller's.
 *
 *   touch:      keys[num_slots] (uint64) and view_mask[num_slots, ceil(V / 32)] (uint32) form an open-addressing table the
 *               call clears itself (empty key = all ones), *overflow (uint32) likewise.  One lane per sampled pixel; a key
 *               is claimed by one 64-bit compare-and-swap, linear probing bounded by num_slots, the view bit set by atomicOr.
 *               When probing is exhausted the insert is dropped, bit 0 of *overflow is set and the inserts still to come are dropped
 *               unprobed: the table is then incomplete in an order-dependent way (the caller doubles num_slots
 *               and repeats); bit 1 is set for a point whose blocks leave [-2^20, 2^20) (or are not finite).  The slot of a
 *               key depends on the order of arrival; the set of keys and their masks do not.
 *   (caller):   keys != empty, sorted ascending, the masks gathered by the same permutation: block_keys[B], view_mask[B, words].
 *   neighbors:  out_nbr[B, 27] int32, entry (dx + 1) 9 + (dy + 1) 3 + (dz + 1) = the rank of block b + (dx, dy, dz) or -1
 *               (binary search in block_keys).
 *   integrate:  out_tsdf[B, 4096], out_weight[B, 4096] (fp32 counts), out_colour[B, 4096, 3] (NULL: views->rgb is not read),
 *               every entry written once.
 *   isosurface_blocks_count_cells / emit_vertices / count_faces / emit_faces: the flag, scan and count contracts of the dense
 *               four over B 4096 cells / lattice points; emit_vertices also writes out_colours[num_vertices, 3] in [0, 1]
 *               unless it or colour is NULL.
 * None synchronises.  SCORP_ERR_INVALID: a NULL pointer (other than the optional ones), num_views < 1 or > 65535, stride < 1,
 * voxel_length <= 0, sdf_trunc <= 0 or > 16 voxel_length, num_slots not a power of two (or > 2^32), num_blocks < 1 or
 * > (2^31 - 1) / 16, more than 2^31 - 1 vertices or quads, a colour output without its input. */
typedef struct ScorpTsdfBlockViews {
  const float *depth;
  const uint8_t *rgb;
  const float *cam;
  int32_t num_views, width, height, _pad;
} ScorpTsdfBlockViews;
int scorp_tsdf_blocks_touch(const ScorpTsdfBlockViews *views, float voxel_length, float sdf_trunc, int32_t stride, uint64_t *keys,
                            uint32_t *view_mask, uint64_t num_slots, uint32_t *overflow, scorp_stream_t stream);
int scorp_tsdf_blocks_neighbors(const uint64_t *block_keys, int64_t num_blocks, int32_t *out_nbr, scorp_stream_t stream);
int scorp_tsdf_blocks_integrate(const ScorpTsdfBlockViews *views, float voxel_length, float sdf_trunc, const uint64_t *block_keys,
                                const uint32_t *view_mask, int64_t num_blocks, float *out_tsdf, float *out_weight,
                                float *out_colour, scorp_stream_t stream);
int scorp_isosurface_blocks_count_cells(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                        uint8_t *out_flags, scorp_stream_t stream);
int scorp_isosurface_blocks_emit_vertices(const float *tsdf, const float *weight, const float *colour, const uint64_t *block_keys,
                                          const int32_t *nbr, int64_t num_blocks, float voxel_length, const int32_t *cell_scan,
                                          int64_t num_vertices, float *out_vertices, float *out_colours, scorp_stream_t stream);
int scorp_isosurface_blocks_count_faces(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                        uint8_t *out_counts, scorp_stream_t stream);
int scorp_isosurface_blocks_emit_faces(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                       const int32_t *cell_scan, const int32_t *edge_scan, int64_t num_quads, int32_t *out_faces,
                                       scorp_stream_t stream);

/* Marching cubes over the same block volume: the rules of scorp_marching_cubes_* applied through block borders, level 0,
 * inside = tsdf < 0, cell validity as above (all eight corners in existing blocks with w > 0).  A lattice edge q -> q + e_a
 * carries a vertex when its ends differ in inside-ness and at least one of the four cells round it is valid (both ends are
 * then valid), so no vertex is left unused at a rim; only valid cells emit triangles.  An edge belongs to the block of q, a
 * cell and its triangles to the block of g.  Vertices come in ascending (block rank, local index of q, axis), triangles in
 * ascending (block rank, local cell index, table order).  Position: voxel_length ((g + 0.5) + t e_a), t = (0 - f0) / (f1 - f0);
 * colour (c0 + t (c1 - c0)) / 255, optional as above.  The mask, count and scan contracts are those of the dense four over
 * B 4096 lattice points / cells.  SCORP_ERR_INVALID as for scorp_isosurface_blocks_*. */
int scorp_marching_cubes_blocks_count_edges(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                            uint8_t *out_masks, uint8_t *out_counts, scorp_stream_t stream);
int scorp_marching_cubes_blocks_emit_vertices(const float *tsdf, const float *weight, const float *colour, const uint64_t *block_keys,
                                              const int32_t *nbr, int64_t num_blocks, float voxel_length, const uint8_t *edge_masks,
                                              const int32_t *edge_scan, int64_t num_vertices, float *out_vertices,
                                              float *out_colours, scorp_stream_t stream);
int scorp_marching_cubes_blocks_count_faces(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                            uint8_t *out_counts, scorp_stream_t stream);
int scorp_marching_cubes_blocks_emit_faces(const float *tsdf, const float *weight, const int32_t *nbr, int64_t num_blocks,
                                           const uint8_t *edge_masks, const int32_t *edge_scan, const int32_t *face_scan,
                                           int64_t num_faces, int32_t *out_faces, scorp_stream_t stream);

/* ---- introspection for stage-level parity tests (device->host copies; synchronises) ---- */
/* xy[N,2], depth[N], conic_opacity[N,4], rgb[N,3], rect[N,4] (tile units, max exclusive); any may be NULL. */
int scorp_gs3d_debug_geom(const void *state, int32_t num_gaussians, int32_t image_width, int32_t image_height,
                          float *xy, float *depth, float *conic_opacity, float *rgb, int32_t *rect,
                          scorp_stream_t stream);
/* Work statistics of the last scorp_gs3d_render on this state: out3[0] = (8x8 block, splat) iterations the blend forward
 * ran (each evaluates 64 pixel-splat pairs: P = 64 * out3[0]), out3[1] = those the blend backward replays (per block, up
 * to its deepest last contributor), out3[2] = number of blocks. */
int scorp_gs3d_debug_work(const void *state, int32_t num_gaussians, int32_t image_width, int32_t image_height,
                          uint64_t *out3, scorp_stream_t stream);
/* tile_start[tiles+1] (uint32) and the sorted splat list point_list[num_pairs] (uint32), both in RASTER tile order
 * (whatever order the lists have in the pair buffer: cell-major under the two-level binning). */
int scorp_gs3d_debug_tiles(const void *state, const void *pairs, uint64_t capacity, int32_t num_gaussians,
                           int32_t image_width, int32_t image_height, uint32_t *tile_start, uint32_t *point_list,
                           scorp_stream_t stream);
/* What the last scorp_gs3d_render (after scorp_gs3d_preprocess) left on this state and pair buffer for the backward:
 * final_T[H*W] (float), n_contrib[H*W] (uint32: per pixel the 1-based position of its last contributor in its 8x8 block's
 * hit list, 0 = none), block_hits[tiles*4] (uint32: hits the block's wave blended; block = tile * 4 + quad, quad = 2 * (lower
 * half) + (right half)) and the four hit-list regions in RASTER tile order like point_list above: with num_pairs =
 * tile_start[tiles] of scorp_gs3d_debug_tiles, entry k of block (t, quad) is out_hits[quad * num_pairs + tile_start[t] + k],
 * out_hits[4 * num_pairs] (uint32 splat ids).  A block's entries are defined up to the largest n_contrib of its pixels (what
 * the backward replays) and undefined beyond.  Any output may be NULL.  Read-only: launches nothing, changes nothing on
 * the device. */
int scorp_gs3d_debug_blend(const void *state, const void *pairs, uint64_t capacity, int32_t num_gaussians,
                           int32_t image_width, int32_t image_height, float *final_T, uint32_t *n_contrib,
                           uint32_t *block_hits, uint32_t *out_hits, scorp_stream_t stream);

/* ---- 2D Gaussian splatting (surfels): replaces diff_surfel_rasterization (gs2dgs/gaussian_renderer/__init__.py:111-120) ----
 * Same ScorpGs3dInputs / ScorpGs3dGrads structs with two reinterpretations: `scales` is [N,2]
 * (gs2dgs/scene/gaussian_model.py:49) and `cov3D_precomp` is the precomputed [N,9] splat->pixel transform
 * (gs2dgs/gaussian_renderer/__init__.py:78-89).  Outputs: color[3,H,W], radii[N], allmap[7,H,W] with channels
 * 0 expected depth (un-normalised), 1 alpha, 2-4 view-space normal, 5 median depth, 6 depth distortion (:131-148).
 * The means2D gradient is the densification statistic the 2DGS model accumulates (gaussian_model.py:495).
 * Pair counting / overflow checks are shared: scorp_gs3d_num_pairs / scorp_gs3d_check_overflow work on this state. */
size_t scorp_gs2d_state_bytes(int32_t num_gaussians, int32_t image_width, int32_t image_height);
size_t scorp_gs2d_backward_scratch_bytes(int32_t num_gaussians);
int scorp_gs2d_preprocess(const ScorpGs3dInputs *in, int32_t *out_radii, void *state, size_t state_bytes,
                          scorp_stream_t stream);
int scorp_gs2d_render(const ScorpGs3dInputs *in, void *state, void *pairs, uint64_t capacity, float *out_color,
                      float *out_allmap, scorp_stream_t stream);
/* As scorp_gs3d_render_image: the same images with nothing left behind for scorp_gs2d_backward. */
int scorp_gs2d_render_image(const ScorpGs3dInputs *in, void *state, void *pairs, uint64_t capacity, float *out_color,
                            float *out_allmap, scorp_stream_t stream);
/* As scorp_gs3d_render_score (same bands, same argument checks, same fixed-order sums), with the surface depth the 2DGS
 * renderer returns (gs2dgs/gaussian_renderer/__init__.py:139-154) in place of depth / alpha:
 *   alpha = allmap[1],  depth = (1 - depth_ratio) * nan_to_num(allmap[0] / alpha, 0, 0) + depth_ratio * nan_to_num(allmap[5], 0, 0),
 *   acc[j] += scale * sum over band j of |alpha - tgt_alpha| + |depth - tgt_depth|,
 * each pixel's term formed with the fp32 operations of that expression in torch.  No colour, normal or distortion is
 * accumulated and no image written.  depth_ratio (PipelineParams.depth_ratio) must be finite and in [0, 1]. */
int scorp_gs2d_render_score(const ScorpGs3dInputs *in, void *state, void *pairs, uint64_t capacity, const float *tgt_depth,
                            const float *tgt_alpha, int32_t rows_per_score, float depth_ratio, float scale, float *acc,
                            scorp_stream_t stream);
int scorp_gs2d_backward(const ScorpGs3dInputs *in, const void *state, const void *pairs, uint64_t capacity,
                        const float *dL_dcolor, const float *dL_dallmap, const ScorpGs3dGrads *grads, void *scratch,
                        size_t scratch_bytes, scorp_stream_t stream);
/* The same with the `flags` of scorp_gs3d_backward_ex.  The surfel backward reduces eight per-pixel values of a hit over
 * the block's pixels on the matrix cores; by default they travel as two fp16 terms each under a per-hit power of two (22
 * bits, exact products, fp32 accumulation).  SCORP_BACKWARD_EXACT_FP32: the values and the upstream gradients stay fp32
 * and the reduction runs on fp32 MFMAs - no operand narrower than the reference's fp32 arithmetic
 * (gs2dgs/gaussian_renderer/__init__.py:111-120 under train_2dgs.py:142-150).  SCORP_BACKWARD_DETERMINISTIC: no float
 * atomics - one plain 80-byte row per (8x8 block, hit) and an ordered per-surfel sum, as in 3-D; two runs give the same bits
 * (utils/mask.py:52-124 votes on signs of repeated backward passes).  SCORP_BACKWARD_SCRATCH_ZEROED is ignored.
 * scratch: scorp_gs2d_backward_scratch_bytes_ex(flags) (num_gaussians * 80 bytes, plus for the deterministic form
 * num_gaussians + 1 pair ordinals, 4 * capacity flag bytes and 4 * capacity rows of 80 bytes). */
size_t scorp_gs2d_backward_scratch_bytes_ex(int32_t num_gaussians, int32_t image_width, int32_t image_height, uint64_t capacity,
                                            uint32_t flags);
int scorp_gs2d_backward_ex(const ScorpGs3dInputs *in, const void *state, const void *pairs, uint64_t capacity,
                           const float *dL_dcolor, const float *dL_dallmap, const ScorpGs3dGrads *grads, void *scratch,
                           size_t scratch_bytes, uint32_t flags, scorp_stream_t stream);
/* T[N,9], xy[N,2], depth[N], normal_opacity[N,4], rgb[N,3], rect[N,4]; any may be NULL (stage-level parity tests). */
int scorp_gs2d_debug_geom(const void *state, int32_t num_gaussians, int32_t image_width, int32_t image_height, float *T,
                          float *xy, float *depth, float *normal_opacity, float *rgb, int32_t *rect,
                          scorp_stream_t stream);

int scorp_gs2d_debug_tiles(const void *state, const void *pairs, uint64_t capacity, int32_t num_gaussians,
                           int32_t image_width, int32_t image_height, uint32_t *tile_start, uint32_t *point_list,
                           scorp_stream_t stream);

/* ---- what render() does to the rasterizer's outputs (gs3dgs/gaussian_renderer/__init__.py:113-120), one launch:
 * out_depth[HW] = nan_to_num(depth / alpha, nan=0, posinf=0); out_visible[N] (bytes, 0/1) = radii > 0.
 * The backward gives dL/ddepth, dL/dalpha for an upstream gradient on out_depth (zeros where alpha = 0). */
int scorp_gs3d_render_tail(const float *depth, const float *alpha, int64_t num_pixels, const int32_t *radii,
                           int32_t num_gaussians, float *out_depth, uint8_t *out_visible, scorp_stream_t stream);
int scorp_gs3d_render_tail_backward(const float *g_out_depth, const float *depth, const float *alpha, int64_t num_pixels,
                                    float *g_depth, float *g_alpha, scorp_stream_t stream);

/* ---- scoring one pose hypothesis against a target view (the render-and-compare form of the rotation sweep,
 * align_3dgs_clpe_9dof.py:80-111 / :336-368), straight from the rasterizer's raw outputs, one launch:
 * acc[0] += scale * sum over the pixels of |alpha - tgt_alpha| + |nan_to_num(depth / alpha, 0, 0) - tgt_depth|
 * (tgt_depth is a NORMALISED depth as scorp_gs3d_render_tail writes it).  One float atomic per workgroup: the order of
 * the partial sums is not fixed. */
int scorp_gs3d_pose_score_accumulate(const float *depth, const float *alpha, const float *tgt_depth, const float *tgt_alpha,
                                     int64_t num_pixels, float scale, float *acc, scorp_stream_t stream);

/* ---- per-pixel tail of the 2DGS render(): gs2dgs/gaussian_renderer/__init__.py:131-160 over
 * gs2dgs/utils/point_utils.py:9-40 (depths_to_points, depth_to_normal) ----
 * allmap[7,H,W] -> render_alpha[1,H,W], render_normal[3,H,W] (rotated to world space by viewmatrix[:3,:3]),
 * render_dist[1,H,W], surf_depth[1,H,W] = expected*(1-depth_ratio) + depth_ratio*median (both nan_to_num(.,0,0)),
 * surf_normal[3,H,W] = normalize(cross(dP/dy, dP/dx)) * alpha with P = surf_depth*rays_d + rays_o, zero on the
 * one-pixel border.  viewmatrix: the camera's world_view_transform (16 floats, as passed to the rasterizer);
 * rays_d[H*W,3] / rays_o[3]: the camera's per-pixel ray table (point_utils.py:9-22).  All pointers are device
 * pointers.  The backward takes the five upstream gradients (any may be NULL = zero) and writes g_allmap[7,H,W];
 * surf_depth is the forward's output.  Where PyTorch's chain yields 0/0 = NaN (empty pixels) it writes 0. */
int scorp_gs2d_maps_forward(int32_t image_width, int32_t image_height, const float *allmap, const float *viewmatrix,
                            const float *rays_d, const float *rays_o, float depth_ratio, float *render_alpha,
                            float *render_normal, float *render_dist, float *surf_depth, float *surf_normal,
                            scorp_stream_t stream);
int scorp_gs2d_maps_backward(int32_t image_width, int32_t image_height, const float *allmap, const float *viewmatrix,
                             const float *rays_d, const float *rays_o, float depth_ratio, const float *surf_depth,
                             const float *g_render_alpha, const float *g_render_normal, const float *g_render_dist,
                             const float *g_surf_depth, const float *g_surf_normal, float *g_allmap,
                             scorp_stream_t stream);

/* ---- the 2DGS regularisers of train_2dgs.py:142-150, fused over the same per-pixel tail ----
 * out2 (device) = { lambda_normal * mean(1 - render_normal . surf_normal), lambda_dist * mean(render_dist) } straight
 * from allmap (no maps are materialised); the backward writes g_allmap[7,H,W] for upstream gradients g_out2 (device,
 * two floats; NULL = ones).  workspace: scorp_gs2d_regularizers_workspace_bytes (per-workgroup partial sums; the
 * reduction order is fixed, so the value is deterministic). */
size_t scorp_gs2d_regularizers_workspace_bytes(int32_t image_width, int32_t image_height);
int scorp_gs2d_regularizers_forward(int32_t image_width, int32_t image_height, const float *allmap, const float *viewmatrix,
                                    const float *rays_d, const float *rays_o, float depth_ratio, float lambda_normal,
                                    float lambda_dist, float *out2, void *workspace, size_t workspace_bytes,
                                    scorp_stream_t stream);
int scorp_gs2d_regularizers_backward(int32_t image_width, int32_t image_height, const float *allmap,
                                     const float *viewmatrix, const float *rays_d, const float *rays_o, float depth_ratio,
                                     float lambda_normal, float lambda_dist, const float *g_out2, float *g_allmap,
                                     scorp_stream_t stream);

/* ---- fused photometric loss (rows a8/a9 of the hot path) ----
 * loss = (1-lambda) * mean|x-y| + lambda * (1 - mean SSIM(x,y)), x = img*mask, y = gt*mask (mask [H,W] or NULL):
 * train_3dgs.py:106-107, post_refine_gs.py:103-111 over gs3dgs/utils/loss_utils.py:17-73 (11x11 Gaussian window,
 * sigma 1.5, zero padding, C1=1e-4, C2=9e-4).  img/gt are [C,H,W].  out_loss3 (device) = {loss, l1, ssim}.
 * The workspace carries the forward's derivative maps to the backward (read-only there). */
size_t scorp_loss_workspace_bytes(int32_t channels, int32_t height, int32_t width);
int scorp_loss_l1_ssim_forward(const float *img, const float *gt, const float *mask, int32_t channels, int32_t height,
                               int32_t width, float lambda_dssim, float *out_loss3, void *workspace,
                               size_t workspace_bytes, int32_t need_backward, scorp_stream_t stream);
/* grad_img[C,H,W] = grad_out[0] * d loss / d img (grad_out: device scalar, NULL = 1). */
int scorp_loss_l1_ssim_backward(const float *img, const float *gt, const float *mask, int32_t channels, int32_t height,
                                int32_t width, float lambda_dssim, const void *workspace, const float *grad_out,
                                float *grad_img, scorp_stream_t stream);

/* ---- one training view in one call (train_3dgs.py:88-150 minus the optimizer: render, photometric loss, backward) ----
 * Enqueues, on `stream` and without any host synchronisation, exactly the sequence a caller of the entry points above
 * would issue for one iteration of the reference's training loop:
 *   scorp_gs3d_preprocess -> scorp_gs3d_render -> scorp_gs3d_render_tail -> scorp_loss_l1_ssim_forward ->
 *   scorp_loss_l1_ssim_backward (upstream gradient 1) -> scorp_gs3d_backward (dL_ddepth = dL_dalpha = NULL).
 * It exists because at ~1 ms of device work per view the host side (Python glue, autograd bookkeeping, a dozen FFI
 * calls) is of the same size: one call keeps the GPU the bottleneck whatever the host is doing.  Every buffer is the
 * caller's, sized as for the separate calls; `capacity` pairs must have been reserved (check with
 * scorp_gs3d_check_overflow afterwards, as for scorp_gs3d_render without scorp_gs3d_num_pairs).
 * out_depth_raw is the rasterizer's un-normalised depth, out_depth = nan_to_num(depth / alpha) as render() returns
 * it; out_depth / out_visible may both be NULL (the tail is skipped then). */
/* Optional optimizer step INSIDE the view (train_3dgs.py:180-193 for the iterations that neither densify nor reset): the
 * per-Gaussian backward kernel holds every Gaussian's whole gradient row in registers / LDS and applies
 * torch.optim.Adam's update there - the arithmetic of scorp_adam_step_guarded, bit for bit - together with the view's share of
 * the densification statistics (scorp_densification_stats' arithmetic).  The 248-byte gradient row never travels to HBM
 * and back and the parameters are not read a second time: 932 instead of 1652 bytes of optimizer traffic per Gaussian.
 * Needs the raw-leaf convention (shs = _features_dc, shs_rest = _features_rest, raw_params = 7, scales + rotations): the
 * arrays of `in` ARE the optimizer's parameters and are updated in place by the view's last kernel.  Leaves in the order
 * xyz, features_dc, features_rest, opacity, scaling, rotation; exp_avg[k] == NULL: that leaf is frozen.  Nothing is updated
 * (and *skipped_counter is incremented, if given) when the view overflowed its pair reservation (the overflow word of
 * out_header, or of the state header) - the guard of scorp_adam_step_guarded, without the host in the loop. */
typedef struct ScorpFusedAdam {
  float *exp_avg[6];
  float *exp_avg_sq[6];
  float lr[6];
  float _pad[2];
  double beta1, beta2, eps;
  int32_t step;                  /* 1-based step count of this update (bias corrections) */
  int32_t _pad2;
  uint32_t *skipped_counter;     /* device word or NULL */
  float *max_radii2D;            /* [N] statistics, all three or none: updated for the visible Gaussians */
  float *xyz_gradient_accum;     /* [N] += |(dL/dmeans2D.x, dL/dmeans2D.y)| */
  float *denom;                  /* [N] += 1 */
} ScorpFusedAdam;

typedef struct ScorpGs3dTrainView {
  const ScorpGs3dInputs *in;
  int32_t *out_radii;            /* [N] */
  void *state;                   /* scorp_gs3d_state_bytes(), 256-byte aligned */
  size_t state_bytes;
  void *pairs;                   /* scorp_gs3d_pairs_bytes(capacity) */
  uint64_t capacity;
  float *out_color;              /* [3,H,W] */
  float *out_depth_raw;          /* [H,W] */
  float *out_alpha;              /* [H,W] */
  float *out_depth;              /* [H,W] or NULL */
  uint8_t *out_visible;          /* [N] bytes or NULL */
  const float *gt;               /* [3,H,W] */
  const float *mask;             /* [H,W] or NULL */
  float lambda_dssim;
  uint32_t backward_flags;       /* flags of scorp_gs3d_backward_ex for the view's backward (SCORP_BACKWARD_EXACT_FP32, ...); 0 = default */
  float *out_loss3;              /* device: {loss, l1, ssim} */
  void *loss_workspace;          /* scorp_loss_workspace_bytes(3, H, W) */
  size_t loss_workspace_bytes;
  float *grad_color;             /* [3,H,W] scratch: d loss / d color */
  const ScorpGs3dGrads *grads;   /* gradients w.r.t. the inputs, as for scorp_gs3d_backward */
  void *backward_scratch;        /* scorp_gs3d_backward_scratch_bytes(N) (scorp_gs3d_backward_scratch_bytes_ex with backward_flags) */
  size_t backward_scratch_bytes;
  uint32_t *out_header;          /* optional, 4 device words {pairs needed, overflow, capacity, 0}: the view's overflow word
                                    survives the state blob without a copy launch (the scatter kernel writes it) */
  const ScorpFusedAdam *adam;    /* optional: the optimizer step and the statistics inside the view (see ScorpFusedAdam) */
} ScorpGs3dTrainView;
int scorp_gs3d_train_view(const ScorpGs3dTrainView *view, scorp_stream_t stream);

/* ---- the loss terms of the late iterations inside the one-call view (train_3dgs.py:109-150, iteration > depth_from_iter) ----
 * With r = nan_to_num(depth_raw / alpha, 0, 0), the depth render() returns (scorp_gs3d_render_tail's arithmetic):
 *   sensor term   (train_3dgs.py:112-120)  Ms = (sensor > SCORP_DEPTH_SENSOR_MIN) & (sensor < SCORP_DEPTH_SENSOR_MAX) & (r > 0),
 *                 Ls = mean over Ms of |r - sensor|;
 *   estimate term (train_3dgs.py:125-134)  Me = (r > 0) & (est > 0), rn = (r - min r) / (max r - min r) and pn likewise from
 *                 est, the extrema taken over Me and not differentiated (image_utils.py:87-91), Le = mean over Me of |rn - pn|;
 *   isotropic     (train_3dgs.py:146-148, loss_utils.py:75-85)  Liso = mean over Gaussians and axes of |s - mean_axes s|,
 *                 s = the activated scales, of the parameters BEFORE this view's optimizer step.
 * out_terms4 (device) = {lambda_depth_sensor Ls + weight_depth_est Le + lambda_isotropic Liso, Ls, Le, Liso}; the caller
 * forms weight_depth_est = 10 * dn_l1_weight(iteration).  A depth term is computed when its map is given; a term that is
 * not computed reports 0.  The gradients with respect to depth_raw and alpha go to grad_depth_raw / grad_alpha (zeros where
 * scorp_gs3d_render_tail_backward writes zeros), which the view hands to its backward; the isotropic gradient
 *   lambda_isotropic / (3 N) * (sgn_j - (sgn_0 + sgn_1 + sgn_2) / 3) * s_j,  sgn = sign(s - mean s),
 * is added to the scaling gradient of EVERY Gaussian, visible or not, by the per-Gaussian backward kernel, before that
 * gradient is written or enters the optimizer step.  No float atomics (per-workgroup partial sums in `workspace`, added in
 * a fixed order): two calls give the same bits.
 * Degenerate inputs: a term whose mask is empty, or whose rendered or estimated depths over Me are all equal (range 0),
 * reports the value NaN - and so does out_terms4[0] - and contributes a ZERO gradient, so that no NaN reaches the
 * parameters or the Adam moments; nothing fails and nothing is written out of bounds.  (The torch formulation raises on an
 * empty Me and yields NaN gradients for the other cases.) */
#define SCORP_DEPTH_SENSOR_MIN 0.3f /* train_3dgs.py:113: the sensor's valid range, exclusive on both sides */
#define SCORP_DEPTH_SENSOR_MAX 7.0f
typedef struct ScorpGs3dViewTerms {
  const float *depth_sensor;     /* [H,W] or NULL */
  const float *depth_est;        /* [H,W] or NULL */
  float lambda_depth_sensor;     /* != 0 needs depth_sensor */
  float weight_depth_est;        /* != 0 needs depth_est */
  float lambda_isotropic;        /* != 0: 3-D scales of the training layout (scales + rotations, shs + shs_rest) */
  float _pad;
  float *out_terms4;             /* device: {weighted sum of the three, Ls, Le, Liso} */
  float *grad_depth_raw;         /* [H,W] scratch, needed with a depth map */
  float *grad_alpha;             /* [H,W] scratch, needed with a depth map */
  void *workspace;               /* scorp_gs3d_view_terms_workspace_bytes(W, H, N), 16-byte aligned */
  size_t workspace_bytes;
} ScorpGs3dViewTerms;
size_t scorp_gs3d_view_terms_workspace_bytes(int32_t width, int32_t height, int32_t num_gaussians);
/* scorp_gs3d_train_view with the terms: between the photometric loss and the backward the view runs the two depth passes
 * and the isotropic value, its backward gets grad_depth_raw / grad_alpha as dL_ddepth / dL_dalpha, and the per-Gaussian
 * backward adds the isotropic gradient.  Total loss of the view = out_loss3[0] + out_terms4[0].  With a depth map the
 * view must produce out_depth.  terms == NULL: scorp_gs3d_train_view, launch for launch.  SCORP_ERR_INVALID before any
 * launch: out_terms4 NULL, a weight without its map, a map without grad_depth_raw / grad_alpha / out_depth, a workspace
 * NULL, misaligned or too small, lambda_isotropic without the training layout. */
int scorp_gs3d_train_view_ex(const ScorpGs3dTrainView *view, const ScorpGs3dViewTerms *terms, scorp_stream_t stream);
/* The two depth terms alone, on caller-given maps (what an autograd front-end wraps): values into out_terms4 (Liso = 0),
 * gradients for an upstream gradient of 1 into grad_depth_raw / grad_alpha [H,W].  At least one map; workspace:
 * scorp_gs3d_view_terms_workspace_bytes(W, H, 0). */
int scorp_gs3d_depth_terms(int32_t width, int32_t height, const float *depth_raw, const float *alpha, const float *depth_sensor,
                           const float *depth_est, float lambda_depth_sensor, float weight_depth_est, float *out_terms4,
                           float *grad_depth_raw, float *grad_alpha, void *workspace, size_t workspace_bytes,
                           scorp_stream_t stream);

/* The 2DGS twin: one iteration of train_2dgs.py:95-150 for the plain photometric loss plus its two regularisers,
 *   scorp_gs2d_preprocess -> scorp_gs2d_render -> scorp_loss_l1_ssim_forward -> scorp_gs2d_regularizers_forward ->
 *   scorp_loss_l1_ssim_backward -> scorp_gs2d_regularizers_backward -> scorp_gs2d_backward,
 * enqueued by one call; total loss = out_loss3[0] + out_reg2[0] + out_reg2[1].  With lambda_normal = lambda_dist = 0
 * (iterations <= 3000, train_2dgs.py:142-143) the regulariser kernels are skipped and no allmap gradient is formed.
 * rays_d[H*W,3] / rays_o[3]: the camera's ray table (see scorp_gs2d_maps_forward).  Every buffer is the caller's. */
typedef struct ScorpGs2dTrainView {
  const ScorpGs3dInputs *in;
  int32_t *out_radii;            /* [N] */
  void *state;                   /* scorp_gs2d_state_bytes(), 256-byte aligned */
  size_t state_bytes;
  void *pairs;                   /* scorp_gs3d_pairs_bytes(capacity) */
  uint64_t capacity;
  float *out_color;              /* [3,H,W] */
  float *out_allmap;             /* [7,H,W] */
  const float *gt;               /* [3,H,W] */
  const float *mask;             /* [H,W] or NULL */
  const float *rays_d;           /* [H*W,3] */
  const float *rays_o;           /* [3] */
  float lambda_dssim, depth_ratio, lambda_normal, lambda_dist;
  float *out_loss3;              /* device: {photometric loss, l1, ssim} */
  float *out_reg2;               /* device: {normal loss, distortion loss} (zeros if both lambdas are 0) */
  void *loss_workspace;          /* scorp_loss_workspace_bytes(3, H, W) */
  size_t loss_workspace_bytes;
  void *reg_workspace;           /* scorp_gs2d_regularizers_workspace_bytes(W, H) */
  size_t reg_workspace_bytes;
  float *grad_color;             /* [3,H,W] scratch */
  float *grad_allmap;            /* [7,H,W] scratch */
  const ScorpGs3dGrads *grads;
  void *backward_scratch;        /* scorp_gs2d_backward_scratch_bytes(N) (scorp_gs2d_backward_scratch_bytes_ex with backward_flags) */
  size_t backward_scratch_bytes;
  uint32_t backward_flags;       /* flags of scorp_gs2d_backward_ex for the view's backward; 0 = default */
  const ScorpFusedAdam *adam;    /* optional: the optimizer step and the statistics inside the view (see ScorpFusedAdam; the
                                    scaling leaf is [N,2], the statistic norms the whole means2D-gradient row) */
} ScorpGs2dTrainView;
int scorp_gs2d_train_view(const ScorpGs2dTrainView *view, scorp_stream_t stream);

/* ---- the loss terms of the late iterations inside the one-call 2DGS view (train_2dgs.py:100-139, iteration > depth_from_iter) ----
 * With d = the surface depth of a pixel as scorp_gs2d_maps_forward forms it (nan_to_num(allmap[0] / allmap[1], 0, 0) and
 * nan_to_num(allmap[5], 0, 0) mixed by depth_ratio: the render_depth of the 2DGS render()):
 *   sensor term   (train_2dgs.py:101-109)  Ls, and
 *   estimate term (train_2dgs.py:114-124)  Le: the definitions, masks, constants and double-precision uniforms of
 *                 ScorpGs3dViewTerms above, with d in place of r;
 *   depth-normal  (train_2dgs.py:126-134)  pred_normal[3,H,W] = the normal of the ESTIMATED depth map through the camera's ray
 *                 table (gs2dgs/utils/point_utils.py:9-37: central differences of the back-projected points, cross product,
 *                 normalised with the epsilon handling of surf_normal, zero on the one-pixel border; not alpha-weighted, no
 *                 gradient),  Ldn = mean over ALL H*W pixels of (1 - surf_normal . pred_normal),  Lrn = the same mean with the
 *                 world-space render_normal; pixels where the estimate is 0 are not masked out;
 *   isotropic     (train_2dgs.py:136-139)  Liso = mean over surfels and both axes of |s - mean_axes s|, s = the activated
 *                 [N,2] scales, of the parameters BEFORE this view's optimizer step.
 * out_terms6 (device) = {lambda_depth_sensor Ls + weight_depth_est Le + weight_depth_normal (Ldn + Lrn) + lambda_isotropic Liso,
 * Ls, Le, Ldn, Lrn, Liso}; the caller forms weight_depth_est = 10 * dn_l1_weight(iteration) and weight_depth_normal =
 * dn_l1_weight(iteration) (0 until depth_from_iter + 1000).  A depth term is computed when its map is given, the depth-normal
 * terms when weight_depth_normal != 0; a term that is not computed reports 0.  Gradients: d loss / d d of the two depth terms
 * goes to grad_depth[H,W], -(weight_depth_normal / HW) pred_normal - the gradient with respect to BOTH surf_normal (its alpha
 * factor stays detached) and render_normal - to grad_normal[3,H,W]; the view's maps backward adds them to the regularisers'
 * gradients and writes all seven channels of grad_allmap once, in one kernel.  The isotropic gradient
 *   lambda_isotropic / (2 N) * (sgn_j - (sgn_0 + sgn_1) / 2) * s_j,  sgn = sign(s - mean s),
 * is added to the scaling gradient of EVERY surfel, visible or not, by the per-surfel backward kernel, before that gradient
 * is written or enters the optimizer step.  No float atomics (per-workgroup partial sums in `workspace`, added in a fixed
 * order): two calls give the same bits.
 * Degenerate inputs: a depth term whose mask is empty, or whose depths over Me are all equal (range 0), reports NaN - and
 * so does out_terms6[0] - and contributes a ZERO gradient; no NaN reaches the parameters or the Adam moments, nothing fails.
 * Ldn and Lrn are plain means over H*W and cannot be empty. */
typedef struct ScorpGs2dViewTerms {
  const float *depth_sensor;     /* [H,W] or NULL */
  const float *depth_est;        /* [H,W] or NULL */
  float lambda_depth_sensor;     /* != 0 needs depth_sensor */
  float weight_depth_est;        /* != 0 needs depth_est */
  float weight_depth_normal;     /* != 0 needs depth_est */
  float lambda_isotropic;        /* != 0: [N,2] scales of the training layout (scales + rotations, shs + shs_rest) */
  float *out_terms6;             /* device: {weighted total, Ls, Le, Ldn, Lrn, Liso} */
  float *out_depth;              /* [H,W]: the surface depth d; needed (and written) with a depth map */
  float *grad_depth;             /* [H,W] scratch, needed with a depth map */
  float *grad_normal;            /* [3,H,W] scratch, needed with weight_depth_normal != 0 */
  void *workspace;               /* scorp_gs2d_view_terms_workspace_bytes(W, H, N), 16-byte aligned */
  size_t workspace_bytes;
} ScorpGs2dViewTerms;
size_t scorp_gs2d_view_terms_workspace_bytes(int32_t width, int32_t height, int32_t num_gaussians);
/* scorp_gs2d_train_view with the terms: between the photometric loss and the backward the view runs the two pixel passes
 * and the isotropic value, its maps backward takes grad_depth / grad_normal next to the regularisers, and the per-surfel
 * backward adds the isotropic gradient.  Total loss of the view = out_loss3[0] + out_reg2[0] + out_reg2[1] + out_terms6[0].
 * With a depth map the view needs rays_d, rays_o and grad_allmap whatever the regularisers' weights.  terms == NULL:
 * scorp_gs2d_train_view, launch for launch.  SCORP_ERR_INVALID before any launch: out_terms6 NULL, a weight without its map,
 * weight_depth_normal without depth_est, a map without out_depth / grad_depth (/ grad_normal) / rays / grad_allmap, a
 * workspace NULL, misaligned or too small, lambda_isotropic without the training layout. */
int scorp_gs2d_train_view_ex(const ScorpGs2dTrainView *view, const ScorpGs2dViewTerms *terms, scorp_stream_t stream);
/* The depth and depth-normal terms alone, on a caller-given allmap (what an autograd front-end wraps): values into
 * out_terms6 (Liso = 0), grad_allmap[7,H,W] for an upstream gradient of 1 (every channel written).  At least one map;
 * out_depth / grad_depth [H,W] and grad_normal [3,H,W] (with weight_depth_normal != 0) are the caller's scratch, as in the
 * struct; workspace: scorp_gs2d_view_terms_workspace_bytes(W, H, 0). */
int scorp_gs2d_surfel_terms(int32_t width, int32_t height, const float *allmap, const float *viewmatrix, const float *rays_d,
                            const float *rays_o, float depth_ratio, const float *depth_sensor, const float *depth_est,
                            float lambda_depth_sensor, float weight_depth_est, float weight_depth_normal, float *out_terms6,
                            float *out_depth, float *grad_depth, float *grad_normal, float *grad_allmap, void *workspace,
                            size_t workspace_bytes, scorp_stream_t stream);

/* ---- rigid / scale transform of a whole model incl. its SH coefficients (utils/gaussians.py:12-108) ----
 * In place, one launch:  xyz <- ((xyz - c) R^T) * s + c + t;  rotation <- q (x) normalize(rotation) (w,x,y,z; q = the
 * quaternion of R);  scaling <- scaling + log(s) (log-space, `scale_dims` = 3, or 2 for surfels);  features_rest
 * [N, rest_coeffs, 3]: band l = 1..3 (coefficients l^2-1 .. (l+1)^2-2 of it) multiplied by the real Wigner-D block D_l.
 * params: 105 device floats, 16-byte aligned: R[9] (row-major) c[3] t[3] s[3] q[4] D1[9] D2[25] D3[49] (D_l row-major;
 * nothing is read behind them).
 * rotation / scaling / features_rest may each be NULL: that part of the model is then left untouched (a translation
 * passes only xyz; the reference's gaussians_translate / gaussians_scale never touch the quaternions). */
int scorp_gaussians_transform(float *xyz, float *rotation, float *scaling, float *features_rest, int32_t num_gaussians,
                              int32_t rest_coeffs, int32_t scale_dims, const float *params, scorp_stream_t stream);

/* ---- simple_knn replacement ----
 * out[i] = mean of the squared distances from point i to its 3 nearest other points, as
 * `simple_knn._C.distCUDA2(points)` (gs3dgs/scene/gaussian_model.py:177).  xyz[N,3], out[N]. */
int scorp_knn_dist2(const float *xyz, int32_t num_points, float *out, scorp_stream_t stream);

/* ---- fused multi-tensor Adam (row a10) ----
 * One launch for all parameter groups of torch.optim.Adam(lr per group, betas, eps=1e-15, no weight decay)
 * (gs3dgs/scene/gaussian_model.py:197-206): m,v moments and parameters updated in place. `step` is the 1-based
 * step count used for the bias corrections. */
#define SCORP_ADAM_MAX_TENSORS 8
typedef struct ScorpAdamTensor {
  float *param;
  const float *grad;
  float *exp_avg;
  float *exp_avg_sq;
  uint64_t numel;
  float lr;
  float _pad;
} ScorpAdamTensor;
int scorp_adam_step(const ScorpAdamTensor *tensors, int32_t num_tensors, double beta1, double beta2, double eps,
                    int32_t step, scorp_stream_t stream);
/* The same step made conditional ON THE DEVICE: nothing is updated if *skip_if_nonzero != 0 when the kernel runs (NULL =
 * unconditional).  For training loops that reserve the pair buffer instead of synchronising for the pair count: the word
 * is the view's overflow flag (second 32-bit word of the forward state), so a view rendered from truncated tile lists
 * cannot move the parameters or the Adam moments - without a host round trip per iteration. */
int scorp_adam_step_guarded(const ScorpAdamTensor *tensors, int32_t num_tensors, double beta1, double beta2, double eps,
                            int32_t step, const uint32_t *skip_if_nonzero, scorp_stream_t stream);

/* The same; when the step is skipped, *skipped_counter (device word, NULL = not counted) is incremented by one - a training loop
 * reads it at its next synchronisation point and takes the skipped steps out of its bias-correction counter.  Replicas of a
 * data-parallel run skip on the all-reduced overflow word, so their counters agree (FusedAdam.take_skipped). */
int scorp_adam_step_guarded_ex(const ScorpAdamTensor *tensors, int32_t num_tensors, double beta1, double beta2, double eps,
                               int32_t step, const uint32_t *skip_if_nonzero, uint32_t *skipped_counter, scorp_stream_t stream);

/* ---- per-view densification statistics (row a11; train_3dgs.py:180-181, train_2dgs.py:189-190,
 * gs3dgs/scene/gaussian_model.py:603-605) ----
 * For every Gaussian i with visible[i] != 0:
 *     max_radii2D[i] = max(max_radii2D[i], (float)radii[i]);
 *     xyz_gradient_accum[i] += sqrt(g[0]^2 + g[1]^2),  g = grad_means2D + i * grad_stride;   denom[i] += 1.
 * One launch instead of the reference's three boolean-mask indexings (each a compaction plus a host synchronisation,
 * ~0.6 ms per iteration at 1 M Gaussians).  Nothing is touched if *skip_if_nonzero != 0 when the kernel runs (NULL =
 * unconditional): the overflow word of a view rendered with a reserved pair buffer, as for scorp_adam_step_guarded. */
int scorp_densification_stats(int32_t num_gaussians, const int32_t *radii, const uint8_t *visible, const float *grad_means2D,
                              int32_t grad_stride, const uint32_t *skip_if_nonzero, float *max_radii2D,
                              float *xyz_gradient_accum, float *denom, scorp_stream_t stream);
/* The same with the gradient norm taken over `norm_components` (2 or 3) leading floats of a row: the 2DGS model's
 * add_densification_stats norms the WHOLE means2D gradient row (gs2dgs/scene/gaussian_model.py:494-495), the 3DGS one
 * only x, y (gs3dgs/scene/gaussian_model.py:603-605).  scorp_densification_stats is this with norm_components = 2. */
int scorp_densification_stats_ex(int32_t num_gaussians, const int32_t *radii, const uint8_t *visible, const float *grad_means2D,
                                 int32_t grad_stride, int32_t norm_components, const uint32_t *skip_if_nonzero,
                                 float *max_radii2D, float *xyz_gradient_accum, float *denom, scorp_stream_t stream);

/* ---- densify / prune compaction (row f2 of the hot-path scope; gs3dgs/scene/gaussian_model.py:412-601) ----
 * Re-indexes up to SCORP_ROWS_MAX_TENSORS row-major float tensors in one launch: dst row j = src row
 * (src_index[j] & 0x7fffffff).  Bit 31 of an index marks a FRESH row (a cloned or split Gaussian): tensors with
 * zero_if_fresh != 0 (the Adam moments) get zeros there instead of a copy.  src and dst must not overlap. */
#define SCORP_ROWS_MAX_TENSORS 24
typedef struct ScorpRowTensor {
  const float *src;
  float *dst;
  uint32_t row_floats;
  uint32_t zero_if_fresh;
} ScorpRowTensor;
int scorp_gather_rows(const ScorpRowTensor *tensors, int32_t num_tensors, const int32_t *src_index, uint64_t num_out_rows,
                      scorp_stream_t stream);

/* ---- in-library kernel timing: hipEvent pairs recorded on the launch stream around every kernel ---- */
/* Off by default. scorp_prof_enable(1) clears the accumulators and starts recording; collect() synchronises the
 * recorded events and returns, per kernel id, the summed duration in ms and the number of launches. */
int scorp_prof_enable(int on);
/* Restrict the bracketing to the kernels whose bit (1 << kernel_id) is set (default: all) — an event pair costs a few
 * microseconds of stream time, so a throughput run brackets only the kernel it reports. */
int scorp_prof_select(uint64_t kernel_mask);
int scorp_prof_num_kernels(void);
const char *scorp_prof_kernel_name(int kernel_id);
int scorp_prof_collect(double *total_ms, uint64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* SCORP_GS_H */
