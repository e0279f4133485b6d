// api.hip — error plumbing and version of libscorp_gs (see include/scorp_gs.h).
#include <stdarg.h>

#include <mutex>
#include <vector>

#include "common.hpp"

namespace scorp {
namespace {
thread_local char g_error[512] = "";
}
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}
}  // namespace scorp

// ---- kernel timing ----
namespace scorp {
bool g_prof_on = false;
uint64_t g_prof_mask = ~0ull;
namespace {
const char *kKernelNames[kKNumKernels] = {"preprocess", "count_tiles", "scan_tiles", "scatter_pairs", "sort_tiles", "blend_forward",
                                          "blend_backward", "preprocess_backward", "ssim_l1_forward", "ssim_l1_backward", "knn_dist2", "adam", "preprocess_2d", "blend_forward_2d",
                                          "blend_backward_2d", "preprocess_backward_2d", "surfel_maps_forward", "surfel_maps_backward"};
struct Pending { hipEvent_t start, stop; int id; };
std::vector<Pending> g_pending;
std::vector<hipEvent_t> g_pool;
std::vector<hipEvent_t> g_open(kKNumKernels, nullptr);
double g_ms[kKNumKernels];
uint64_t g_count[kKNumKernels];
std::mutex g_mu;
hipEvent_t get_event() {
  if (!g_pool.empty()) { hipEvent_t e = g_pool.back(); g_pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
}  // namespace
void prof_begin(int id, hipStream_t stream) {
  if (!((g_prof_mask >> id) & 1)) return;
  std::lock_guard<std::mutex> lk(g_mu);
  hipEvent_t e = get_event();
  (void)hipEventRecord(e, stream);
  g_open[id] = e;
}
void prof_end(int id, hipStream_t stream) {
  if (!((g_prof_mask >> id) & 1)) return;
  std::lock_guard<std::mutex> lk(g_mu);
  hipEvent_t e = get_event();
  (void)hipEventRecord(e, stream);
  g_pending.push_back({g_open[id], e, id});
  g_open[id] = nullptr;
}
}  // namespace scorp

extern "C" int scorp_prof_enable(int on) {
  std::lock_guard<std::mutex> lk(scorp::g_mu);
  for (auto &p : scorp::g_pending) { scorp::g_pool.push_back(p.start); scorp::g_pool.push_back(p.stop); }
  scorp::g_pending.clear();
  for (int k = 0; k < scorp::kKNumKernels; k++) { scorp::g_ms[k] = 0; scorp::g_count[k] = 0; }
  scorp::g_prof_on = on != 0;
  return SCORP_OK;
}
extern "C" int scorp_prof_select(uint64_t kernel_mask) {
  std::lock_guard<std::mutex> lk(scorp::g_mu);
  scorp::g_prof_mask = kernel_mask;
  return SCORP_OK;
}
extern "C" int scorp_prof_num_kernels(void) { return scorp::kKNumKernels; }
extern "C" const char *scorp_prof_kernel_name(int k) {
  return (k >= 0 && k < scorp::kKNumKernels) ? scorp::kKernelNames[k] : "";
}
extern "C" int scorp_prof_collect(double *total_ms, uint64_t *launches) {
  std::lock_guard<std::mutex> lk(scorp::g_mu);
  for (auto &p : scorp::g_pending) {
    hipError_t e = hipEventSynchronize(p.stop);
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, p.start, p.stop);
    if (e != hipSuccess) { scorp::set_error("event timing failed: %s", hipGetErrorString(e)); return SCORP_ERR_HIP; }
    scorp::g_ms[p.id] += ms;
    scorp::g_count[p.id] += 1;
    scorp::g_pool.push_back(p.start);
    scorp::g_pool.push_back(p.stop);
  }
  scorp::g_pending.clear();
  for (int k = 0; k < scorp::kKNumKernels; k++) {
    if (total_ms) total_ms[k] = scorp::g_ms[k];
    if (launches) launches[k] = scorp::g_count[k];
  }
  return SCORP_OK;
}

extern "C" int scorp_version(void) { return 102; /* 0.1.2: scorp_icp_point_to_point */ }

#ifndef SCORP_SOURCE_SHA
#define SCORP_SOURCE_SHA "unknown"
#endif
// sha256 (first 16 hex digits) of the kernel sources this library was built from (scorp_amd/build.py): lets bench.py
// tell whether the PMC-derived figures under profiles/ were collected on the code that is running
extern "C" const char *scorp_source_sha(void) { return SCORP_SOURCE_SHA; }
extern "C" const char *scorp_last_error(void) { return scorp::g_error; }

// ---- the checks and layouts every kind shares ----
namespace scorp {
int validate(const GsKind &K, const ScorpGs3dInputs *in, int *views) {
  if (!in) { set_error("inputs is NULL"); return SCORP_ERR_INVALID; }
  if (in->num_gaussians < 0 || in->image_width <= 0 || in->image_height <= 0) {
    set_error("bad sizes: N=%d W=%d H=%d", in->num_gaussians, in->image_width, in->image_height);
    return SCORP_ERR_INVALID;
  }
  if (in->image_width > 16 * 65535 || in->image_height > 16 * 65535) {   // (BinRec holds tile rectangles as uint16)
    set_error("image larger than 65535 tiles per axis"); return SCORP_ERR_INVALID;
  }
  if (in->num_gaussians > 0) {
    if (!in->means3D || !in->opacities) { set_error("means3D / opacities is NULL"); return SCORP_ERR_INVALID; }
    if (in->shs_rest && !in->shs) { set_error("shs_rest given without shs (the degree-0 block)"); return SCORP_ERR_INVALID; }
    if ((in->shs == nullptr) == (in->colors_precomp == nullptr)) {
      set_error("provide exactly one of shs / colors_precomp"); return SCORP_ERR_INVALID;
    }
    const bool sr = in->scales != nullptr && in->rotations != nullptr;
    if (sr == (in->cov3D_precomp != nullptr) || ((in->scales != nullptr) != (in->rotations != nullptr))) {
      set_error("provide exactly one of scales+rotations / cov3D_precomp"); return SCORP_ERR_INVALID;
    }
    if (in->shs) {
      if (in->sh_degree < 0 || in->sh_degree > 3) { set_error("sh_degree %d not in 0..3", in->sh_degree); return SCORP_ERR_INVALID; }
      if (in->sh_coeffs < (in->sh_degree + 1) * (in->sh_degree + 1)) {
        set_error("sh_coeffs %d < (sh_degree+1)^2", in->sh_coeffs); return SCORP_ERR_INVALID;
      }
    }
  }
  if (!in->bg || !in->viewmatrix || !in->projmatrix || !in->campos) {
    set_error("bg / viewmatrix / projmatrix / campos is NULL"); return SCORP_ERR_INVALID;
  }
  *views = 1;
  if (K.stacked_views) {
    if (in->num_views < 0) { set_error("num_views %d is negative", in->num_views); return SCORP_ERR_INVALID; }
    if (in->num_views > 1) {
      const long long nt = (long long)in->num_views * in->num_gaussians, ht = (long long)in->num_views * in->image_height;
      if (in->image_height % kTile != 0) { set_error("num_views > 1 needs image_height to be a multiple of %d", kTile); return SCORP_ERR_INVALID; }
      if (nt > 0x7FFFFFFFll || ht > 16 * 65535ll) { set_error("num_views x N or num_views x H too large"); return SCORP_ERR_INVALID; }
      if (K.mode2d && in->cov3D_precomp) {   // (a surfel's given transform maps to ONE view's pixels)
        set_error("num_views > 1 with cov3D_precomp: a given 2DGS transform is view dependent"); return SCORP_ERR_INVALID;
      }
      *views = in->num_views;
    }
  }
  // SH rows and quaternions are fetched as 16-byte words (and SH rows by direct global -> LDS loads)
  if ((((uintptr_t)in->shs | (uintptr_t)in->shs_rest | (uintptr_t)in->rotations) & 15) != 0) {
    set_error("shs / shs_rest / rotations must be 16-byte aligned"); return SCORP_ERR_INVALID;
  }
  return SCORP_OK;
}

int check_buffers(const void *state, const void *pairs, uint64_t capacity) {
  if (!state || ((uintptr_t)state & 255) || !pairs || ((uintptr_t)pairs & 255)) {
    set_error("state / pairs buffer NULL or not 256-byte aligned"); return SCORP_ERR_INVALID;
  }
  if (capacity > 0xFFFFFFFFull) { set_error("capacity above 2^32-1 pairs"); return SCORP_ERR_INVALID; }
  return SCORP_OK;
}

int read_header(const void *state, hipStream_t stream, StateHeader *h) {
  SCORP_HIP_CHECK(hipMemcpyAsync(h, state, sizeof(*h), hipMemcpyDeviceToHost, stream));
  SCORP_HIP_CHECK(hipStreamSynchronize(stream));
  return SCORP_OK;
}

int render_frame(const GsKind &K, const ScorpGs3dInputs *in, void *state, void *pairs, uint64_t capacity, bool for_backward,
                 RenderFrame *f) {
  int V;
  if (int e = validate(K, in, &V)) return e;
  if (V > 1 && for_backward) {
    set_error("num_views > 1 is forward only: use %s", K.mode2d ? "scorp_gs2d_render_image" : "scorp_gs3d_render_image");
    return SCORP_ERR_INVALID;
  }
  if (int e = check_buffers(state, pairs, capacity)) return e;
  const int N = V * in->num_gaussians, W = in->image_width, H = V * in->image_height;
  *f = {V, N, W, H, (uint32_t)capacity, StateLayout(N, W, H, K.mode2d, V), PairLayout(capacity), (char *)state, (char *)pairs};
  return SCORP_OK;
}
}  // namespace scorp

int scorp::copy_geom_to_host(const void *state, const StateLayout &L, int N, size_t rec_bytes, void **rec, const BinRec **bin,
                             hipStream_t stream) {
  if (!state) { set_error("state is NULL"); return SCORP_ERR_INVALID; }
  *rec = nullptr;
  *bin = nullptr;
  if (N <= 0) return SCORP_OK;
  char *h = (char *)malloc((size_t)N * (rec_bytes + sizeof(BinRec)));
  if (!h) { set_error("host allocation failed"); return SCORP_ERR_INVALID; }
  hipError_t e = hipMemcpyAsync(h, (const char *)state + L.rec, (size_t)N * rec_bytes, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h + (size_t)N * rec_bytes, (const char *)state + L.bin, (size_t)N * sizeof(BinRec), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) { free(h); set_error("debug_geom copy failed: %s", hipGetErrorString(e)); return SCORP_ERR_HIP; }
  *rec = h;
  *bin = (const BinRec *)(h + (size_t)N * rec_bytes);
  return SCORP_OK;
}
