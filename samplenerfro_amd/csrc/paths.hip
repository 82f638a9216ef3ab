// Bent-path diagnostics: per-ray reductions of the march records (rnerf_path_summary) and polylines of selected rays drawn into
// orthographic panels as finished bytes (rnerf_path_plot).  Reference: extract_mesh.py:178-225 (the bent path of one pixel, pickled and
// drawn from four directions by plt_utils.plot_path) and the per-pixel map eval.py:173,195 carries commented out
// (`any(|idx_grad| > 1e-3 along the path)`, mask_{idx}.png).  include/rnerf.h has the specification; tests/helpers/paths_ref.py restates
// it in numpy.  Records are float4 [num_nodes][B] as rnerf_march writes them.
#include "common.h"
#include "eval_host.h"

#include <math.h>

namespace rnerf {

constexpr int PATH_AHEAD = 8;          // nodes whose loads one lane keeps in flight (two batches of this many: 2 x 8 x 32 B per lane)
constexpr int PLOT_MAX_PANELS = 8;
constexpr unsigned PLOT_ID_MASK = 0x0FFFFFFFu;
enum { PLOT_BOX = 1, PLOT_SHADOW = 2, PLOT_PATH = 3, PLOT_MARKER = 4 };

__device__ __forceinline__ float sumsq3(float a, float b, float c) { return fadd(fadd(fmul(a, a), fmul(b, b)), fmul(c, c)); }
// |grad n| > eps, strict; a NaN norm compares false
__device__ __forceinline__ bool refracting(const float4 ior, float eps) { return fsqrt(sumsq3(ior.y, ior.z, ior.w)) > eps; }

struct PathAcc { int count, first, last; double optical; };

// node k with its successor's position: the refracting test of k and the term (n_k - 1) * |x_k - x_{k+1}| of the optical thickness
__device__ __forceinline__ void path_node(PathAcc& a, int k, const float4 p, const float4 pn, const float4 ior, float eps) {
  if (refracting(ior, eps)) { ++a.count; a.first = a.first < 0 ? k : a.first; a.last = k; }
  const float len = fsqrt(sumsq3(fsub(p.x, pn.x), fsub(p.y, pn.y), fsub(p.z, pn.z)));
  a.optical = __dadd_rn(a.optical, __dmul_rn((double)fsub(ior.x, 1.0f), (double)len));
}

// One ray per lane, nodes serial: every load of a wave is one contiguous 1 KiB row of the [node][B] layout.  The float64 sum has a
// fixed order (ascending k), so a ray is not split over lanes; the loads of the next PATH_AHEAD nodes are issued before the current
// PATH_AHEAD are consumed.  One wave per workgroup: a chunk of 8192 rays is only 128 waves, which then spread over 128 CUs.
__global__ void __launch_bounds__(64) path_summary_kernel(const float4* __restrict__ pd, const float4* __restrict__ dr, const float4* __restrict__ ior,
                                                          int N, int B, float eps, int* __restrict__ nodes, float* __restrict__ maps) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= B) return;
  const size_t row = (size_t)B;
  const float4* pdr = pd + r;
  const float4* ir = ior + r;
  const int M = N - 1;                                   // segments
  PathAcc a{0, -1, -1, 0.0};
  float4 p = pdr[0];
  float4 P[PATH_AHEAD], I[PATH_AHEAD], Pn[PATH_AHEAD], In[PATH_AHEAD];
  int k0 = 0;
  if (PATH_AHEAD <= M) {
#pragma unroll
    for (int u = 0; u < PATH_AHEAD; ++u) { P[u] = pdr[(size_t)(u + 1) * row]; I[u] = ir[(size_t)u * row]; }
  }
  for (; k0 + PATH_AHEAD <= M; k0 += PATH_AHEAD) {
    const bool more = k0 + 2 * PATH_AHEAD <= M;          // the same in every lane
    if (more) {
#pragma unroll
      for (int u = 0; u < PATH_AHEAD; ++u) {
        Pn[u] = pdr[(size_t)(k0 + PATH_AHEAD + u + 1) * row];
        In[u] = ir[(size_t)(k0 + PATH_AHEAD + u) * row];
      }
    }
#pragma unroll
    for (int u = 0; u < PATH_AHEAD; ++u) { path_node(a, k0 + u, p, P[u], I[u], eps); p = P[u]; }
    if (more) {
#pragma unroll
      for (int u = 0; u < PATH_AHEAD; ++u) { P[u] = Pn[u]; I[u] = In[u]; }
    }
  }
  for (; k0 < M; ++k0) {                                  // fewer than PATH_AHEAD segments left
    const float4 pn = pdr[(size_t)(k0 + 1) * row];
    path_node(a, k0, p, pn, ir[(size_t)k0 * row], eps);
    p = pn;
  }
  if (refracting(ir[(size_t)M * row], eps)) { ++a.count; a.first = a.first < 0 ? M : a.first; a.last = M; }
  const float4 d0 = dr[r], d1 = dr[(size_t)M * row + r];
  nodes[r] = a.count; nodes[row + r] = a.first; nodes[2 * row + r] = a.last;
  maps[r] = fsqrt(sumsq3(fsub(d1.x, d0.x), fsub(d1.y, d0.y), fsub(d1.z, d0.z)));
  maps[row + r] = (float)a.optical;
}

// ---- the plot -------------------------------------------------------------------------------------------------------------------------
struct PlotPanels { double m[PLOT_MAX_PANELS][2][4]; };
struct PlotBox { double lo[3], hi[3]; int on; };
struct PlotPix { long long x, y; bool ok; };

__device__ __forceinline__ double plot_dot(const double* m, double x, double y, double z) {
  return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[0], x), __dmul_rn(m[1], y)), __dmul_rn(m[2], z)), m[3]);
}
// the pixel of a point: (floor(u), floor(v)); not drawable when u or v is not finite or reaches 2^30 in magnitude
__device__ __forceinline__ PlotPix plot_pixel(const double (*m)[4], double x, double y, double z) {
  const double u = plot_dot(m[0], x, y, z), v = plot_dot(m[1], x, y, z);
  PlotPix q;
  q.ok = fabs(u) < 1073741824.0 && fabs(v) < 1073741824.0;          // false for NaN and the infinities
  q.x = q.ok ? (long long)floor(u) : 0;
  q.y = q.ok ? (long long)floor(v) : 0;
  return q;
}
__device__ __forceinline__ long long floor_div(long long a, long long b) {      // b > 0
  const long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
__device__ __forceinline__ void plot_put(unsigned* __restrict__ keys, int size, long long x, long long y, unsigned key) {
  if (x >= 0 && x < size && y >= 0 && y < size) atomicMax(keys + (size_t)y * size + (size_t)x, key);
}
// Pixel i of n + 1, n = max(|dx|, |dy|): (x0 + floor((2 i dx + n) / (2 n)), y0 + floor((2 i dy + n) / (2 n))).  Along the major axis
// that is x0 +- i exactly, so i is cut to the range whose major coordinate lies inside the panel: at most `size` iterations.
__device__ void plot_segment(unsigned* __restrict__ keys, int size, const PlotPix a, const PlotPix b, unsigned key) {
  if (!(a.ok && b.ok)) return;
  const long long dx = b.x - a.x, dy = b.y - a.y;
  const long long adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
  const long long n = adx > ady ? adx : ady;
  if (n == 0) { plot_put(keys, size, a.x, a.y, key); return; }
  const bool xmajor = adx >= ady;
  const long long c0 = xmajor ? a.x : a.y, dc = xmajor ? dx : dy;          // |dc| = n
  long long i0, i1;
  if (dc > 0) { i0 = -c0; i1 = (long long)size - 1 - c0; } else { i0 = c0 - ((long long)size - 1); i1 = c0; }
  i0 = i0 < 0 ? 0 : i0;
  i1 = i1 > n ? n : i1;
  const long long n2 = 2 * n;
  for (long long i = i0; i <= i1; ++i)
    plot_put(keys, size, a.x + floor_div(2 * i * dx + n, n2), a.y + floor_div(2 * i * dy + n, n2), key);
}

// Item t < num_nodes * R is node k = t / R of ray slot j = t % R: in every panel the path segment k -> k + 1, its shadow on z = floor_z
// and the 3 x 3 marker of node k.  The 12 items after those are the box edges.  A grid-stride loop over the items.
__global__ void __launch_bounds__(256) path_plot_draw_kernel(const float4* __restrict__ pd, const float4* __restrict__ ior, int N, int B,
                                                             const int* __restrict__ rays, int R, PlotPanels pan, int P, int size, PlotBox box,
                                                             double floor_z, int shadow, float eps, unsigned* __restrict__ keys) {
  const long long n_path = (long long)N * R, items = n_path + (box.on ? 12 : 0);
  const size_t panel = (size_t)size * size;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < items; t += (long long)gridDim.x * blockDim.x) {
    if (t >= n_path) {
      const int e = (int)(t - n_path), ax = e >> 2, bx = (ax + 1) % 3, cx = (ax + 2) % 3;
      double s[3], f[3];                                  // edge e runs along axis e / 4; bits 0 and 1 of e pick the side on the next two axes
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const bool high = (i == bx && (e & 1)) || (i == cx && (e & 2));
        s[i] = (i == ax || !high) ? box.lo[i] : box.hi[i];
        f[i] = i == ax ? box.hi[i] : s[i];
      }
      for (int p = 0; p < P; ++p)
        plot_segment(keys + p * panel, size, plot_pixel(pan.m[p], s[0], s[1], s[2]), plot_pixel(pan.m[p], f[0], f[1], f[2]),
                     ((unsigned)PLOT_BOX << 28) | (unsigned)e);
      continue;
    }
    const int k = (int)(t / R), j = (int)(t % R);
    const int ray = rays[j];
    if (ray < 0 || ray >= B) continue;
    const float4 a = pd[(size_t)k * B + ray];
    const bool seg = k + 1 < N;
    const float4 b = seg ? pd[(size_t)(k + 1) * B + ray] : a;
    const bool mark = ior != nullptr && refracting(ior[(size_t)k * B + ray], eps);
    for (int p = 0; p < P; ++p) {
      unsigned* kp = keys + p * panel;
      const PlotPix qa = plot_pixel(pan.m[p], (double)a.x, (double)a.y, (double)a.z);
      if (seg) {
        plot_segment(kp, size, qa, plot_pixel(pan.m[p], (double)b.x, (double)b.y, (double)b.z), ((unsigned)PLOT_PATH << 28) | (unsigned)j);
        if (shadow)
          plot_segment(kp, size, plot_pixel(pan.m[p], (double)a.x, (double)a.y, floor_z), plot_pixel(pan.m[p], (double)b.x, (double)b.y, floor_z),
                       ((unsigned)PLOT_SHADOW << 28) | (unsigned)j);
      }
      if (mark && qa.ok)
        for (int oy = -1; oy <= 1; ++oy)
          for (int ox = -1; ox <= 1; ++ox) plot_put(kp, size, qa.x + ox, qa.y + oy, ((unsigned)PLOT_MARKER << 28) | (unsigned)j);
    }
  }
}

__global__ void __launch_bounds__(256) path_plot_resolve_kernel(const unsigned* __restrict__ keys, long long npix, const uint8_t* __restrict__ ray_rgb,
                                                                uint8_t* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npix) return;
  const unsigned key = keys[i], layer = key >> 28, id = key & PLOT_ID_MASK;
  uint8_t r = 255, g = 255, b = 255;                                        // background
  if (layer == PLOT_BOX) { r = 255; g = 0; b = 0; }
  else if (layer == PLOT_SHADOW) { r = 139; g = 206; b = 151; }
  else if (layer == PLOT_PATH) { r = ray_rgb[3 * (size_t)id]; g = ray_rgb[3 * (size_t)id + 1]; b = ray_rgb[3 * (size_t)id + 2]; }
  else if (layer == PLOT_MARKER) { r = 0; g = 0; b = 0; }
  out[3 * i] = r; out[3 * i + 1] = g; out[3 * i + 2] = b;
}

static bool plot_shape(int32_t P, int32_t size) { return P >= 1 && P <= PLOT_MAX_PANELS && size >= 1 && size <= 8192; }
static const char* const PLOT_SHAPE_MSG = "need 1 <= P <= 8 panels of 1 <= size <= 8192";

}  // namespace rnerf

using namespace rnerf;

extern "C" int rnerf_path_summary(const float* path_pd, const float* path_dr, const float* path_ior, int32_t num_nodes, int32_t B, double grad_eps,
                                  int32_t* nodes, float* maps, void* stream) {
  RNERF_CHECK_ARG(path_pd && path_dr && path_ior && nodes && maps, "rnerf_path_summary: null pointer");
  RNERF_CHECK_ARG(num_nodes >= 1 && B >= 1, "rnerf_path_summary: need num_nodes >= 1 and B >= 1");
  RNERF_CHECK_ARG((((uintptr_t)path_pd | (uintptr_t)path_dr | (uintptr_t)path_ior) & 15) == 0 && (((uintptr_t)nodes | (uintptr_t)maps) & 3) == 0,
                  "rnerf_path_summary: the records must be 16-byte, nodes and maps 4-byte aligned");
  RNERF_CHECK_ARG(!isnan(grad_eps), "rnerf_path_summary: grad_eps is NaN");
  hipLaunchKernelGGL(path_summary_kernel, dim3((unsigned)(((int64_t)B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const float4*)path_pd,
                     (const float4*)path_dr, (const float4*)path_ior, num_nodes, B, (float)grad_eps, nodes, maps);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" size_t rnerf_path_plot_workspace_bytes(int32_t P, int32_t size) {
  if (!plot_shape(P, size)) {
    set_error("rnerf_path_plot_workspace_bytes: %s", PLOT_SHAPE_MSG);
    return 0;
  }
  return up16((size_t)P * size * size * sizeof(uint32_t));
}

extern "C" int rnerf_path_plot(const float* path_pd, const float* path_ior, int32_t num_nodes, int32_t B, const int32_t* rays, const uint8_t* ray_rgb,
                               int32_t R, const double* panels, int32_t P, int32_t size, const double* box, double floor_z, double grad_eps,
                               void* workspace, uint8_t* out, void* stream) {
  RNERF_CHECK_ARG(panels && workspace && out, "rnerf_path_plot: null pointer (panels, workspace, out)");
  RNERF_CHECK_ARG(plot_shape(P, size), "rnerf_path_plot: %s", PLOT_SHAPE_MSG);
  RNERF_CHECK_ARG(R >= 0 && R <= (int32_t)PLOT_ID_MASK, "rnerf_path_plot: need 0 <= R < 2^28 rays");
  RNERF_CHECK_ARG(R == 0 || (path_pd && rays && ray_rgb && num_nodes >= 1 && B >= 1),
                  "rnerf_path_plot: null pointer (path_pd, rays, ray_rgb) or num_nodes, B < 1 with R > 0");
  RNERF_CHECK_ARG((((uintptr_t)path_pd | (uintptr_t)path_ior) & 15) == 0 && (((uintptr_t)rays | (uintptr_t)workspace) & 3) == 0,
                  "rnerf_path_plot: the records must be 16-byte, rays and workspace 4-byte aligned");
  RNERF_CHECK_ARG(!isnan(grad_eps), "rnerf_path_plot: grad_eps is NaN");
  PlotPanels pan;
  for (int p = 0; p < P; ++p)
    for (int i = 0; i < 8; ++i) pan.m[p][i / 4][i % 4] = panels[8 * p + i];
  PlotBox bx;
  bx.on = box != nullptr;
  for (int i = 0; i < 3; ++i) { bx.lo[i] = box ? box[i] : 0.0; bx.hi[i] = box ? box[3 + i] : 0.0; }
  hipStream_t st = (hipStream_t)stream;
  unsigned* keys = (unsigned*)workspace;
  const long long npix = (long long)P * size * size;
  RNERF_CHECK_HIP(hipMemsetAsync(keys, 0, (size_t)npix * sizeof(uint32_t), st));
  const long long items = (long long)(R ? num_nodes : 0) * R + (bx.on ? 12 : 0);
  if (items > 0) {
    const long long blocks = (items + 255) / 256;
    hipLaunchKernelGGL(path_plot_draw_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, (const float4*)path_pd,
                       (const float4*)path_ior, R ? num_nodes : 0, B, rays, R, pan, P, size, bx, floor_z, isnan(floor_z) ? 0 : 1, (float)grad_eps,
                       keys);
  }
  hipLaunchKernelGGL(path_plot_resolve_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, (const unsigned*)keys, npix, ray_rgb, out);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}
