// mesh_render.hip — a z-buffer rasterizer for triangle meshes: depth, face, barycentric and colour maps of a mesh from any
// number of cameras, and the number of views in which each face owns a pixel (scorp_amd/mesh/render.py; the rules are the
// numbered mesh-render block of include/scorp_gs.h, tests/mesh_render_reference.py restates them with exact integers and
// fractions).
//
//   project  one thread per (view, vertex): the float64 projection and the snap to 1/256 pixel, 16 bytes per vertex
//            (X, Y, 1 / w; 1 / w = 0 marks a vertex that drops its triangles), so a vertex is transformed once per view.
//   small    one thread per (view, face): set-up in int64, the box of pixel centres clipped to the image.  A box of at most
//            kMeshRenderSmallBox centres is walked by the thread; any other face goes to the view's large list through an
//            integer counter (the order of the list decides nothing: the minimum does).
//   large    workgroups stride over the view's list, a workgroup's threads over the clipped box of one triangle.  The list
//            holds F entries per view, so it cannot overflow, and its length is read from the device counter: no host
//            read-back anywhere in the call.
//   resolve  one thread per (view, pixel): the winning key back to depth and face, the barycentrics and the colour from
//            the same set-up, and the per-view flag of the face for the visibility count.
//   count    one thread per face: the view flags summed onto out_visible_views.
// Coverage is exact integer arithmetic, the depth float64 with contraction off, the z-buffer one 64-bit unsigned atomicMin
// per candidate (an ordinary vector global atomic): the maps are a function of the inputs alone.  Every loop runs over a box
// clipped to the image.  No kernel spills or uses LDS (tests/test_mesh_render_resources.py).  The face load, the bounds of a
// mesh and their checks are mesh_common.hpp's.
#include "mesh_common.hpp"

namespace scorp {
namespace {

constexpr int kMeshRenderThreads = 256;
constexpr int kMeshRenderSmallBox = 64;        // pixel centres a single thread walks; a larger box goes to the large list
constexpr int kMeshRenderLargeGroups = 1024;   // workgroups per view that stride over the large list
constexpr int kMeshRenderMaxViews = 65535;     // the views are the grid's y dimension
constexpr int kMeshRenderMaxSide = 16384;
constexpr double kMeshRenderSnapLimit = 536870912.0;   // 2^29, in units of 1/256 pixel (rule 2)
constexpr unsigned long long kMeshRenderEmpty = ~0ull;

struct ProjVert {   // rules 1 and 2 for one (view, vertex)
  int32_t X, Y;     // the snapped position in 1/256 pixel, |X|, |Y| <= 2^29
  double inv_w;     // 1 / w > 0, or 0: a triangle with this vertex is dropped for the view
};
static_assert(sizeof(ProjVert) == 16, "ProjVert must be 16 bytes");

struct MeshRenderLayout {
  size_t proj, keys, list, count, flags, bytes;
  MeshRenderLayout(int64_t Nv, int64_t F, int64_t V, int64_t H, int64_t W) {
    size_t off = 0;
    count = off; off = align_up(off + (size_t)V * 4, 256);   // first: the caller may read the lists' lengths back from here
    proj = off; off = align_up(off + (size_t)V * (size_t)Nv * sizeof(ProjVert), 256);
    keys = off; off = align_up(off + (size_t)V * (size_t)H * (size_t)W * 8, 256);
    list = off; off = align_up(off + (size_t)V * (size_t)F * 4, 256);
    flags = off; off = align_up(off + (size_t)V * (size_t)F, 256);
    bytes = off;
  }
};

bool mesh_render_sizes_ok(int64_t Nv, int64_t F, int64_t V, int64_t H, int64_t W) {
  return Nv >= 1 && Nv <= kMeshMaxVertices && F >= 0 && F <= kMeshMaxFaces && V >= 1 && V <= kMeshRenderMaxViews && H >= 1 &&
         H <= kMeshRenderMaxSide && W >= 1 && W <= kMeshRenderMaxSide;
}

// One triangle of one view after rule 3: the corners in LOCAL order (the face's own, or with corners 1 and 2 exchanged
// when the face's own order has A < 0), A > 0.
struct Tri {
  int64_t x0, y0, x1, y1, x2, y2;
  double iw0, iw1, iw2;
  int64_t A;
  int32_t i0, i1, i2;   // the face's own vertex indices
  bool swapped;
};

// The edge function of the edge a -> b at P: positive on the inner side of a triangle with A > 0.
__device__ __forceinline__ int64_t edge_fn(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t px, int64_t py) {
  return (by - ay) * (px - ax) - (bx - ax) * (py - ay);
}
// rule 4: a -> b is a left edge (it runs down the image) or a top edge (it is level and runs towards smaller x)
__device__ __forceinline__ bool top_left(int64_t ax, int64_t ay, int64_t bx, int64_t by) {
  return by - ay > 0 || (by - ay == 0 && bx - ax < 0);
}
__device__ __forceinline__ bool owns(int64_t e, bool tl) { return e > 0 || (e == 0 && tl); }

// rules 2 (the drops) and 3; false: the face is dropped for this view
__device__ __forceinline__ bool tri_setup(const int32_t *__restrict__ faces, int32_t Nv, const ProjVert *__restrict__ pv, int64_t f,
                                          uint32_t flags, Tri &t) {
  const Face face = load_face(faces, f, Nv);
  t.i0 = face.a;
  t.i1 = face.b;
  t.i2 = face.c;
  if (!face.ok) return false;
  const ProjVert a = pv[t.i0], b = pv[t.i1], c = pv[t.i2];
  if (!(a.inv_w > 0.0) || !(b.inv_w > 0.0) || !(c.inv_w > 0.0)) return false;
  t.x0 = a.X; t.y0 = a.Y; t.iw0 = a.inv_w;
  t.x1 = b.X; t.y1 = b.Y; t.iw1 = b.inv_w;
  t.x2 = c.X; t.y2 = c.Y; t.iw2 = c.inv_w;
  t.A = edge_fn(t.x0, t.y0, t.x1, t.y1, t.x2, t.y2);
  if (t.A == 0) return false;
  t.swapped = t.A < 0;
  if (t.swapped) {
    if (flags & SCORP_MESH_RENDER_CULL_BACKFACES) return false;
    t.x1 = c.X; t.y1 = c.Y; t.iw1 = c.inv_w;
    t.x2 = b.X; t.y2 = b.Y; t.iw2 = b.inv_w;
    t.A = -t.A;
  }
  return true;
}

// the pixel centres [i0, i1] x [j0, j1] inside the triangle's bounding box and the image; false when there is none
__device__ __forceinline__ bool tri_box(const Tri &t, int W, int H, int &i0, int &i1, int &j0, int &j1) {
  const int64_t xmin = min(t.x0, min(t.x1, t.x2)), xmax = max(t.x0, max(t.x1, t.x2));
  const int64_t ymin = min(t.y0, min(t.y1, t.y2)), ymax = max(t.y0, max(t.y1, t.y2));
  const int64_t a = max((xmin + 255) >> 8, (int64_t)0), b = min(xmax >> 8, (int64_t)W - 1);   // ceil and floor of x / 256
  const int64_t c = max((ymin + 255) >> 8, (int64_t)0), d = min(ymax >> 8, (int64_t)H - 1);
  if (a > b || c > d) return false;
  i0 = (int)a; i1 = (int)b; j0 = (int)c; j1 = (int)d;
  return true;
}

struct TriEdges {
  bool tl0, tl1, tl2;
};
__device__ __forceinline__ TriEdges tri_edges(const Tri &t) {
  return {top_left(t.x1, t.y1, t.x2, t.y2), top_left(t.x2, t.y2, t.x0, t.y0), top_left(t.x0, t.y0, t.x1, t.y1)};
}
__device__ __forceinline__ void tri_eval(const Tri &t, int i, int j, int64_t &e0, int64_t &e1, int64_t &e2) {
  const int64_t px = (int64_t)i << 8, py = (int64_t)j << 8;
  e0 = edge_fn(t.x1, t.y1, t.x2, t.y2, px, py);
  e1 = edge_fn(t.x2, t.y2, t.x0, t.y0, px, py);
  e2 = edge_fn(t.x0, t.y0, t.x1, t.y1, px, py);
}
__device__ __forceinline__ double tri_q(const Tri &t, int64_t e0, int64_t e1, int64_t e2) {
#pragma clang fp contract(off)
  return ((double)e0 * t.iw0 + (double)e1 * t.iw1) + (double)e2 * t.iw2;
}

// rules 4 and 5 for one pixel centre
__device__ __forceinline__ void tri_pixel(const Tri &t, const TriEdges &tl, int i, int j, uint32_t f, unsigned long long *__restrict__ keys,
                                          int W) {
#pragma clang fp contract(off)
  int64_t e0, e1, e2;
  tri_eval(t, i, j, e0, e1, e2);
  if (!(owns(e0, tl.tl0) && owns(e1, tl.tl1) && owns(e2, tl.tl2))) return;
  const float depth = (float)((double)t.A / tri_q(t, e0, e1, e2));
  const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | f;
  unsigned long long *slot = keys + ((size_t)j * W + i);
  if (key < __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMin(slot, key);   // (the read only spares atomics: the minimum is the same)
}

// rules 1 and 2
__global__ void __launch_bounds__(kMeshRenderThreads) mesh_render_project_kernel(const float *__restrict__ verts, int64_t Nv,
                                                                                  const float *__restrict__ full_proj, int H, int W,
                                                                                  double near, ProjVert *__restrict__ proj) {
#pragma clang fp contract(off)
  const int64_t n = (int64_t)blockIdx.x * kMeshRenderThreads + threadIdx.x;
  if (n >= Nv) return;
  const int v = blockIdx.y;
  const float *m = full_proj + 16 * (size_t)v;
  const double x = (double)verts[3 * n], y = (double)verts[3 * n + 1], z = (double)verts[3 * n + 2];
  const double p0 = (z * (double)m[8] + (y * (double)m[4] + x * (double)m[0])) + (double)m[12];
  const double p1 = (z * (double)m[9] + (y * (double)m[5] + x * (double)m[1])) + (double)m[13];
  const double w = (z * (double)m[11] + (y * (double)m[7] + x * (double)m[3])) + (double)m[15];
  const double inv_w = 1.0 / w;
  const double sx = ((p0 * inv_w + 1.0) * (double)W - 1.0) * 0.5;
  const double sy = ((p1 * inv_w + 1.0) * (double)H - 1.0) * 0.5;
  const double fx = floor(sx * 256.0 + 0.5), fy = floor(sy * 256.0 + 0.5);
  const bool ok = w > near && w < __builtin_inf() && fabs(fx) <= kMeshRenderSnapLimit && fabs(fy) <= kMeshRenderSnapLimit;   // (a NaN fails)
  ProjVert out;
  out.X = ok ? (int32_t)fx : 0;
  out.Y = ok ? (int32_t)fy : 0;
  out.inv_w = ok ? inv_w : 0.0;
  proj[(size_t)v * (size_t)Nv + (size_t)n] = out;
}

__global__ void __launch_bounds__(kMeshRenderThreads) mesh_render_small_kernel(const int32_t *__restrict__ faces, int64_t F, int32_t Nv,
                                                                                const ProjVert *__restrict__ proj, int H, int W,
                                                                                uint32_t flags, unsigned long long *__restrict__ keys,
                                                                                uint32_t *__restrict__ list, uint32_t *__restrict__ count) {
  const int64_t f = (int64_t)blockIdx.x * kMeshRenderThreads + threadIdx.x;
  if (f >= F) return;
  const int v = blockIdx.y;
  Tri t;
  if (!tri_setup(faces, Nv, proj + (size_t)v * (size_t)Nv, f, flags, t)) return;
  int i0, i1, j0, j1;
  if (!tri_box(t, W, H, i0, i1, j0, j1)) return;
  if ((int64_t)(i1 - i0 + 1) * (int64_t)(j1 - j0 + 1) > kMeshRenderSmallBox) {
    const uint32_t pos = atomicAdd(&count[v], 1u);
    if (pos < (uint32_t)F) list[(size_t)v * (size_t)F + pos] = (uint32_t)f;   // (every face enters at most once: always true)
    return;
  }
  const TriEdges tl = tri_edges(t);
  unsigned long long *view_keys = keys + (size_t)v * (size_t)H * (size_t)W;
  for (int j = j0; j <= j1; j++)
    for (int i = i0; i <= i1; i++) tri_pixel(t, tl, i, j, (uint32_t)f, view_keys, W);
}

__global__ void __launch_bounds__(kMeshRenderThreads) mesh_render_large_kernel(const int32_t *__restrict__ faces, int64_t F, int32_t Nv,
                                                                                const ProjVert *__restrict__ proj, int H, int W,
                                                                                uint32_t flags, unsigned long long *__restrict__ keys,
                                                                                const uint32_t *__restrict__ list,
                                                                                const uint32_t *__restrict__ count) {
  const int v = blockIdx.y;
  const uint32_t n = min(count[v], (uint32_t)F);
  unsigned long long *view_keys = keys + (size_t)v * (size_t)H * (size_t)W;
  for (uint32_t e = blockIdx.x; e < n; e += gridDim.x) {
    const uint32_t f = list[(size_t)v * (size_t)F + e];
    if (f >= (uint32_t)F) continue;
    Tri t;
    int i0, i1, j0, j1;
    if (!tri_setup(faces, Nv, proj + (size_t)v * (size_t)Nv, f, flags, t) || !tri_box(t, W, H, i0, i1, j0, j1)) continue;
    const TriEdges tl = tri_edges(t);
    const uint32_t bw = (uint32_t)(i1 - i0 + 1), cells = bw * (uint32_t)(j1 - j0 + 1);   // at most 2^28
    for (uint32_t c = threadIdx.x; c < cells; c += kMeshRenderThreads)
      tri_pixel(t, tl, i0 + (int)(c % bw), j0 + (int)(c / bw), f, view_keys, W);
  }
}

// rules 6 and 7
__global__ void __launch_bounds__(kMeshRenderThreads) mesh_render_resolve_kernel(
    const int32_t *__restrict__ faces, int64_t F, int32_t Nv, const ProjVert *__restrict__ proj, const float *__restrict__ colors, int H,
    int W, uint32_t flags, const unsigned long long *__restrict__ keys, const float *__restrict__ support_depth, float support_tolerance,
    float *__restrict__ out_depth, int32_t *__restrict__ out_face, float *__restrict__ out_bary, float *__restrict__ out_color,
    uint8_t *__restrict__ view_flags) {
#pragma clang fp contract(off)
  const size_t hw = (size_t)H * (size_t)W;
  const size_t p = (size_t)blockIdx.x * kMeshRenderThreads + threadIdx.x;
  if (p >= hw) return;
  const int v = blockIdx.y;
  const size_t at = (size_t)v * hw + p;
  const unsigned long long key = keys[at];
  const uint32_t f = (uint32_t)key;
  Tri t;
  float depth = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
  int32_t face = -1;
  if (key != kMeshRenderEmpty && f < (uint32_t)F && tri_setup(faces, Nv, proj + (size_t)v * (size_t)Nv, f, flags, t)) {
    depth = __uint_as_float((uint32_t)(key >> 32));
    face = (int32_t)f;
    if (out_bary || out_color) {
      int64_t e0, e1, e2;
      tri_eval(t, (int)(p % (size_t)W), (int)(p / (size_t)W), e0, e1, e2);
      const double q = tri_q(t, e0, e1, e2);
      const double l0 = ((double)e0 * t.iw0) / q, l1 = ((double)e1 * t.iw1) / q, l2 = ((double)e2 * t.iw2) / q;
      const double w0 = l0, w1 = t.swapped ? l2 : l1, w2 = t.swapped ? l1 : l2;   // back to the face's own order
      b0 = (float)w0; b1 = (float)w1; b2 = (float)w2;
      if (out_color) {
        const float *c0 = colors + 3 * (size_t)t.i0, *c1 = colors + 3 * (size_t)t.i1, *c2 = colors + 3 * (size_t)t.i2;
        cr = (float)((w0 * (double)c0[0] + w1 * (double)c1[0]) + w2 * (double)c2[0]);
        cg = (float)((w0 * (double)c0[1] + w1 * (double)c1[1]) + w2 * (double)c2[1]);
        cb = (float)((w0 * (double)c0[2] + w1 * (double)c1[2]) + w2 * (double)c2[2]);
      }
    }
    if (view_flags) {
      bool counts = true;
      if (support_depth) {
        const float s = support_depth[at];
        counts = s > 0.0f && fabsf(depth - s) <= support_tolerance;
      }
      if (counts) view_flags[(size_t)v * (size_t)F + f] = 1;   // (many threads, one value)
    }
  }
  out_depth[at] = depth;
  out_face[at] = face;
  if (out_bary) {
    float *o = out_bary + (size_t)v * 3 * hw + p;
    o[0] = b0; o[hw] = b1; o[2 * hw] = b2;
  }
  if (out_color) {
    float *o = out_color + (size_t)v * 3 * hw + p;
    o[0] = cr; o[hw] = cg; o[2 * hw] = cb;
  }
}

__global__ void __launch_bounds__(kMeshRenderThreads) mesh_render_count_kernel(const uint8_t *__restrict__ view_flags, int64_t F, int V,
                                                                                int32_t *__restrict__ out_visible_views) {
  const int64_t f = (int64_t)blockIdx.x * kMeshRenderThreads + threadIdx.x;
  if (f >= F) return;
  int32_t n = 0;
  for (int v = 0; v < V; v++) n += view_flags[(size_t)v * (size_t)F + (size_t)f];
  out_visible_views[f] += n;
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" size_t scorp_mesh_render_workspace_bytes(int64_t num_vertices, int64_t num_faces, int32_t num_views, int32_t height,
                                                    int32_t width) {
  if (!mesh_render_sizes_ok(num_vertices, num_faces, num_views, height, width)) return 0;
  return MeshRenderLayout(num_vertices, num_faces, num_views, height, width).bytes;
}

extern "C" int scorp_mesh_render(const float *vertices, int64_t num_vertices, const int32_t *faces, int64_t num_faces, const float *colors,
                                 const float *full_proj, int32_t num_views, int32_t height, int32_t width, double near, uint32_t flags,
                                 const float *support_depth, float support_tolerance, float *out_depth, int32_t *out_face,
                                 float *out_barycentric, float *out_color, int32_t *out_visible_views, void *workspace,
                                 size_t workspace_bytes, scorp_stream_t stream) {
  if (int e = check_vertices(num_vertices, "mesh_render", true)) return e;
  if (int e = check_faces(num_faces, "mesh_render", 0, true)) return e;
  if (num_views < 1 || num_views > kMeshRenderMaxViews) { set_error("mesh_render: num_views must be in [1, 65535]; got %d", num_views); return SCORP_ERR_INVALID; }
  if (height < 1 || height > kMeshRenderMaxSide || width < 1 || width > kMeshRenderMaxSide) { set_error("mesh_render: height and width must be in [1, 16384]; got %d x %d", height, width); return SCORP_ERR_INVALID; }
  if (!(near > 0.0) || !(near < __builtin_inf())) { set_error("mesh_render: near must be positive and finite"); return SCORP_ERR_INVALID; }
  if (flags & ~(uint32_t)SCORP_MESH_RENDER_CULL_BACKFACES) { set_error("mesh_render: unknown flags 0x%x", flags); return SCORP_ERR_INVALID; }
  if (!vertices || !full_proj || !out_depth || !out_face || (num_faces > 0 && !faces)) { set_error("mesh_render: NULL argument"); return SCORP_ERR_INVALID; }
  if (out_color && !colors) { set_error("mesh_render: out_color without colors"); return SCORP_ERR_INVALID; }
  if (support_depth && !(support_tolerance >= 0.0f)) { set_error("mesh_render: support_tolerance must not be negative or NaN"); return SCORP_ERR_INVALID; }
  const MeshRenderLayout L(num_vertices, num_faces, num_views, height, width);
  if (!workspace || workspace_bytes < L.bytes || ((uintptr_t)workspace & 255)) {
    set_error("mesh_render: workspace NULL, too small or not 256-byte aligned (%zu < %zu)", workspace_bytes, L.bytes);
    return SCORP_ERR_INVALID;
  }
  hipStream_t s = (hipStream_t)stream;
  char *w = (char *)workspace;
  ProjVert *proj = (ProjVert *)(w + L.proj);
  unsigned long long *keys = (unsigned long long *)(w + L.keys);
  uint32_t *list = (uint32_t *)(w + L.list), *count = (uint32_t *)(w + L.count);
  uint8_t *view_flags = out_visible_views && num_faces > 0 ? (uint8_t *)(w + L.flags) : nullptr;
  const size_t hw = (size_t)height * (size_t)width;
  const int32_t Nv = (int32_t)num_vertices;
  SCORP_HIP_CHECK(hipMemsetAsync(keys, 0xFF, (size_t)num_views * hw * 8, s));   // the clear of rule 5: every key all ones
  SCORP_HIP_CHECK(hipMemsetAsync(count, 0, (size_t)num_views * 4, s));
  if (num_faces > 0) {
    if (view_flags) SCORP_HIP_CHECK(hipMemsetAsync(view_flags, 0, (size_t)num_views * (size_t)num_faces, s));
    mesh_render_project_kernel<<<dim3(blocks_for((size_t)num_vertices, kMeshRenderThreads), (unsigned)num_views), kMeshRenderThreads, 0, s>>>(
        vertices, num_vertices, full_proj, height, width, near, proj);
    SCORP_KERNEL_CHECK("mesh_render_project", 0, s);
    mesh_render_small_kernel<<<dim3(blocks_for((size_t)num_faces, kMeshRenderThreads), (unsigned)num_views), kMeshRenderThreads, 0, s>>>(
        faces, num_faces, Nv, proj, height, width, flags, keys, list, count);
    SCORP_KERNEL_CHECK("mesh_render_small", 0, s);
    const unsigned groups = (unsigned)(num_faces < kMeshRenderLargeGroups ? num_faces : kMeshRenderLargeGroups);
    mesh_render_large_kernel<<<dim3(groups, (unsigned)num_views), kMeshRenderThreads, 0, s>>>(faces, num_faces, Nv, proj, height, width,
                                                                                             flags, keys, list, count);
    SCORP_KERNEL_CHECK("mesh_render_large", 0, s);
  }
  mesh_render_resolve_kernel<<<dim3(blocks_for(hw, kMeshRenderThreads), (unsigned)num_views), kMeshRenderThreads, 0, s>>>(
      faces, num_faces, Nv, proj, colors, height, width, flags, keys, support_depth, support_tolerance, out_depth, out_face, out_barycentric,
      out_color, view_flags);
  SCORP_KERNEL_CHECK("mesh_render_resolve", 0, s);
  if (view_flags) {
    mesh_render_count_kernel<<<blocks_for((size_t)num_faces, kMeshRenderThreads), kMeshRenderThreads, 0, s>>>(view_flags, num_faces, num_views,
                                                                                                 out_visible_views);
    SCORP_KERNEL_CHECK("mesh_render_count", 0, s);
  }
  return SCORP_OK;
}
