// Visual-hull carving: the IoR grid of a captured scene from its object masks.
// Reference: calib/make_visual_hull.py:107-146 (main's voxel grid, projection loop and mesh.pkl values), :30-44 (project_2d).
// The reference builds a [G, G, G, 4] float64 point array and runs einsum / divide / round / clip / fancy-index over it once per view on
// the host.  Here a workgroup owns a 4 x 4 x 16 brick of voxels (z fastest across lanes), loops over the views with each voxel's count
// in a register and stores it once: no atomics, no float reductions, the same integers on every run.
#include "common.h"

#include <math.h>

namespace rnerf {

// Voxel centres as make_visual_hull.py:112-120 forms them in float64: np.linspace(0, 1, G)[i] * (max - min) + min, with
// np.linspace's i * (1 / (G - 1)) and its last element set to 1.0 (as vox_coord of grid.hip).
struct HullGrid { int G; double step, mn[3], span[3]; };
__device__ __forceinline__ double hull_coord(const HullGrid& hg, int axis, int i) {
  const double lin = (i == hg.G - 1) ? 1.0 : i * hg.step;
  return lin * hg.span[axis] + hg.mn[axis];
}

constexpr int HULL_BX = 4, HULL_BY = 4, HULL_BZ = 16;      // brick of one 256-thread workgroup; one wave = one x slab of 4 x 16

// masks uint8 [rows][W] (rows = V * H) -> one bit per pixel, `wpr` = ceil(W / 32) words per row, bit (px & 31) of word px >> 5 set where
// the mask is > 0 (cv2.imread(...)[..., 0] > 0, make_visual_hull.py:126,132).  One wave packs 64 pixels of a row with a ballot; the bits
// past W of a row's last word are 0.
__global__ void __launch_bounds__(256) hull_pack_kernel(const uint8_t* __restrict__ masks, long long rows, int W, int wpr,
                                                        uint32_t* __restrict__ bits) {
  const int lane = threadIdx.x & 63;
  const long long spr = (W + 63) / 64, total = rows * spr;
  const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
  for (long long seg = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); seg < total; seg += nwaves) {
    const long long row = seg / spr;
    const int s = (int)(seg % spr), px = s * 64 + lane;
    const bool on = px < W && masks[row * W + px] > 0;
    const unsigned long long b = __ballot(on);
    const int word = 2 * s + lane;
    if (lane < 2 && word < wpr) bits[row * wpr + word] = (uint32_t)(b >> (32 * lane));
  }
}

// make_visual_hull.py:125-134 for one brick.  pv: double[V][12], row-major 3 x 4 p_mat @ view_mat of each view (uniform across the
// wave: scalar loads).  (a, b, c) = pv @ (x, y, z, 1) as individually rounded multiplies and adds (-ffp-contract=off), u = a / c and
// v = b / c, np.round = round half even, np.clip to the image.  There is no test of the sign of c, as in the reference.  NaN and
// +-inf (c == 0, a non-finite transform) clamp to an in-range pixel: fmax(NaN, 0) is 0.
// The two IEEE divisions are the expensive instructions.
__global__ void __launch_bounds__(256) hull_count_kernel(const uint32_t* __restrict__ bits, const double* __restrict__ pv, int V, int H,
                                                         int W, int wpr, HullGrid hg, int accumulate, int* __restrict__ count) {
  const int t = threadIdx.x;
  const int k = blockIdx.x * HULL_BZ + (t & (HULL_BZ - 1));
  const int j = blockIdx.y * HULL_BY + ((t >> 4) & (HULL_BY - 1));
  const int i = blockIdx.z * HULL_BX + (t >> 6);
  if (i >= hg.G || j >= hg.G || k >= hg.G) return;
  const double x = hull_coord(hg, 0, i), y = hull_coord(hg, 1, j), z = hull_coord(hg, 2, k);
  const double wmax = (double)(W - 1), hmax = (double)(H - 1);
  const size_t view_words = (size_t)H * wpr;
  int c = 0;
  for (int v = 0; v < V; ++v) {
    const double* p = pv + (size_t)v * 12;
    const double a = ((p[0] * x + p[1] * y) + p[2] * z) + p[3];
    const double b = ((p[4] * x + p[5] * y) + p[6] * z) + p[7];
    const double d = ((p[8] * x + p[9] * y) + p[10] * z) + p[11];
    const double ru = rint(a / d), rv = rint(b / d);
    const int us = (int)fmin(fmax(ru, 0.0), wmax), vs = (int)fmin(fmax(rv, 0.0), hmax);      // in [0, W - 1] x [0, H - 1]: fmax(NaN, 0) is 0
    const uint32_t word = bits[(size_t)v * view_words + (size_t)vs * wpr + (us >> 5)];
    c += (int)((word >> (us & 31)) & 1u);
  }
  const size_t idx = ((size_t)i * hg.G + j) * hg.G + k;
  count[idx] = accumulate ? count[idx] + c : c;
}

// make_visual_hull.py:136,141: count / num_imgs > threshold in float64, then the grid value.
__global__ void hull_finalize_kernel(const int* __restrict__ count, long long n, double views, double threshold, double ior_in,
                                     double ior_out, float* __restrict__ out) {
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n) return;
  out[id] = (float)(((double)count[id] / views > threshold) ? ior_in : ior_out);
}

static bool hull_grid(const rnerf_grid* g, HullGrid* out) {
  if (!(g->dims[0] == g->dims[1] && g->dims[1] == g->dims[2] && g->dims[0] >= 2)) return false;
  const long long G = g->dims[0];
  if (G * G * G >= (1LL << 31)) return false;
  HullGrid hg;
  hg.G = (int)G;
  hg.step = 1.0 / (double)(G - 1);
  for (int a = 0; a < 3; ++a) { hg.mn[a] = g->nmin[a]; hg.span[a] = g->nmax[a] - g->nmin[a]; }
  *out = hg;
  return true;
}

static bool hull_mask_shape(int64_t V, int32_t H, int32_t W) {
  return V >= 1 && V < (1LL << 31) && H >= 1 && W >= 1 && (int64_t)H * W < (1LL << 31);
}

}  // namespace rnerf

using namespace rnerf;

extern "C" size_t rnerf_visual_hull_workspace_bytes(int64_t num_views, int32_t height, int32_t width) {
  if (!hull_mask_shape(num_views, height, width)) {
    set_error("rnerf_visual_hull_workspace_bytes: need 1 <= num_views < 2^31, height, width >= 1, height * width < 2^31");
    return 0;
  }
  return (size_t)num_views * (size_t)height * (size_t)((width + 31) / 32) * sizeof(uint32_t);
}

extern "C" int rnerf_visual_hull_pack(const uint8_t* masks, int64_t num_views, int32_t height, int32_t width, void* workspace, void* stream) {
  RNERF_CHECK_ARG(masks && workspace, "rnerf_visual_hull_pack: null pointer");
  RNERF_CHECK_ARG(hull_mask_shape(num_views, height, width),
                  "rnerf_visual_hull_pack: need 1 <= num_views < 2^31, height, width >= 1, height * width < 2^31");
  RNERF_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "rnerf_visual_hull_pack: workspace must be 4-byte aligned");
  const long long rows = (long long)num_views * height, segs = rows * ((width + 63) / 64);
  const long long blocks = (segs + 3) / 4;
  hipLaunchKernelGGL(hull_pack_kernel, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, (hipStream_t)stream, masks, rows,
                     width, (width + 31) / 32, (uint32_t*)workspace);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_visual_hull_count(const uint8_t* masks, int64_t num_views, int32_t height, int32_t width, const double* pv,
                                       const rnerf_grid* g, int32_t accumulate, int32_t* count, void* workspace, void* stream) {
  RNERF_CHECK_ARG(pv && g && count && workspace, "rnerf_visual_hull_count: null pointer");
  RNERF_CHECK_ARG(hull_mask_shape(num_views, height, width),
                  "rnerf_visual_hull_count: need 1 <= num_views < 2^31, height, width >= 1, height * width < 2^31");
  HullGrid hg;
  RNERF_CHECK_ARG(hull_grid(g, &hg), "rnerf_visual_hull_count: cubic grids only, 2 <= num_voxels, num_voxels^3 < 2^31");
  RNERF_CHECK_ARG(accumulate == 0 || accumulate == 1, "rnerf_visual_hull_count: accumulate must be 0 or 1");
  RNERF_CHECK_ARG(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)pv & 7) == 0, "rnerf_visual_hull_count: workspace must be 4-byte, pv 8-byte aligned");
  if (masks) {                                                  // null: the workspace already holds these views' bits (rnerf_visual_hull_pack)
    int rc = rnerf_visual_hull_pack(masks, num_views, height, width, workspace, stream);
    if (rc != RNERF_OK) return rc;
  }
  const int G = hg.G;
  hipLaunchKernelGGL(hull_count_kernel, dim3((G + HULL_BZ - 1) / HULL_BZ, (G + HULL_BY - 1) / HULL_BY, (G + HULL_BX - 1) / HULL_BX), dim3(256), 0,
                     (hipStream_t)stream, (const uint32_t*)workspace, pv, (int)num_views, height, width, (width + 31) / 32, hg, accumulate, count);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_visual_hull_finalize(const int32_t* count, const rnerf_grid* g, int64_t total_views, double threshold, double ior_inside,
                                          double ior_outside, float* out, void* stream) {
  RNERF_CHECK_ARG(count && g && out, "rnerf_visual_hull_finalize: null pointer");
  HullGrid hg;
  RNERF_CHECK_ARG(hull_grid(g, &hg), "rnerf_visual_hull_finalize: cubic grids only, 2 <= num_voxels, num_voxels^3 < 2^31");
  RNERF_CHECK_ARG(total_views >= 1, "rnerf_visual_hull_finalize: total_views must be >= 1");
  const long long n = (long long)hg.G * hg.G * hg.G;
  hipLaunchKernelGGL(hull_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, count, n, (double)total_views,
                     threshold, ior_inside, ior_outside, out);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}
