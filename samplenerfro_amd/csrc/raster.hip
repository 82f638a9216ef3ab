// Mesh silhouettes: first-surface depth of a triangle mesh from a pinhole view, and the box dilation + bounding rectangle of the mask.
// Reference: metric/render_mask.py:84-94 (pyrender's depth buffer, `depth != 0`, cv2.dilate with a 35 x 35 box), read back by
// metric/summary.py:177-205 (MASK / CROP).  pyrender needs OpenGL; here the mesh is rasterised with the camera model of
// generate_rays_kernel (render.hip) and the fp64 top-left containment test of voxel_columns_kernel (grid.hip), include/rnerf.h has the
// specification.  Launches of rnerf_mesh_depth: project the vertices; per face the range of 16 x 16 pixel tiles its bounding box meets
// and the per-tile counts; a fixed-order scan; the fill of the per-tile lists through a cursor; the pixel kernel.  A face that meets more
// than RASTER_SMALL tiles goes to one list every tile walks instead (the workspace is then bounded by the mesh, not by the view).  The
// atomics decide the ORDER of a list only; depth is a minimum, tri a minimum among equals and hits a count, so no output sees that order.
#include "common.h"
#include "eval_host.h"

#include <math.h>

namespace rnerf {

constexpr int RASTER_TILE = 16;        // pixels per tile side: one 256-thread workgroup, one wave64 per 8 x 8 quadrant
constexpr int RASTER_SMALL = 4;        // a face whose bounding box meets at most this many tiles is binned per tile
constexpr int RASTER_TB = 128;         // faces staged through LDS per batch

// ri: the float64 inverse (raster_camera) of the float32 rotation R of the camera-to-world, row-major — not its transpose: a float32
// rotation is orthogonal to about 1e-8 only, and the pixel's ray is t + lambda R cam.  t widened from float32; fx .. pc rounded to
// float32 first, as rnerf_generate_rays holds them.  sy, sz: the signs of the camera's y and view axes (Blender: -1, -1; OpenCV: +1, +1).
struct RasterCam { double ri[9], t[3], fx, fy, cx, cy, pc, sy, sz; };

// proj[v] = (X, Y, w): the image-plane point in pixel units (pixel (row, col) samples (col + pc, row + pc)) and w = 1 / depth,
// depth = the distance along the view axis.  w = 0 marks a vertex that cannot be drawn (depth <= 0, or a non-finite projection).
__global__ void __launch_bounds__(256) raster_project_kernel(const double* __restrict__ verts, long long V, RasterCam c, double* __restrict__ proj) {
  const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const double d0 = verts[3 * v] - c.t[0], d1 = verts[3 * v + 1] - c.t[1], d2 = verts[3 * v + 2] - c.t[2];
  const double xc = (c.ri[0] * d0 + c.ri[1] * d1) + c.ri[2] * d2;              // R^-1 (p - t)
  const double yc = (c.ri[3] * d0 + c.ri[4] * d1) + c.ri[5] * d2;
  const double zc = (c.ri[6] * d0 + c.ri[7] * d1) + c.ri[8] * d2;
  const double depth = c.sz * zc;
  const double X = (xc * c.fx) / depth + c.cx, Y = ((c.sy * yc) * c.fy) / depth + c.cy, w = 1.0 / depth;
  const bool ok = depth > 0.0 && isfinite(X) && isfinite(Y) && isfinite(w) && w > 0.0;
  proj[3 * v] = X; proj[3 * v + 1] = Y; proj[3 * v + 2] = ok ? w : 0.0;
}

// first / last pixel index whose sample coordinate i + pc can lie in [lo, hi], widened by one pixel (the edge functions decide, this only
// bounds the work) and clamped to [0, n] / [-1, n - 1]: an empty range has first > last
__device__ __forceinline__ int raster_first(double lo, double pc, int n) { return (int)fmin(fmax(ceil(lo - pc) - 1.0, 0.0), (double)n); }
__device__ __forceinline__ int raster_last(double hi, double pc, int n) { return (int)fmin(fmax(floor(hi - pc) + 1.0, -1.0), (double)(n - 1)); }

// fbox[f] = (tx0, ty0, tx1, ty1), the inclusive tile range of face f; tx1 < tx0 where the face draws nothing.
__global__ void __launch_bounds__(256) raster_face_kernel(const int* __restrict__ faces, long long F, const double* __restrict__ proj, int H, int W,
                                                          int ntx, double pc, int4* __restrict__ fbox, int* __restrict__ tile_count,
                                                          int* __restrict__ large_count, int* __restrict__ large_list,
                                                          unsigned long long* __restrict__ skipped) {
  const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const double* A = proj + 3 * (long long)faces[3 * f], *B = proj + 3 * (long long)faces[3 * f + 1], *C = proj + 3 * (long long)faces[3 * f + 2];
  int4 box = make_int4(0, 0, -1, -1);
  if (A[2] == 0.0 || B[2] == 0.0 || C[2] == 0.0) {
    atomicAdd(skipped, 1ull);
  } else {
    const int c0 = raster_first(fmin(fmin(A[0], B[0]), C[0]), pc, W), c1 = raster_last(fmax(fmax(A[0], B[0]), C[0]), pc, W);
    const int r0 = raster_first(fmin(fmin(A[1], B[1]), C[1]), pc, H), r1 = raster_last(fmax(fmax(A[1], B[1]), C[1]), pc, H);
    if (c0 <= c1 && r0 <= r1) {
      box = make_int4(c0 / RASTER_TILE, r0 / RASTER_TILE, c1 / RASTER_TILE, r1 / RASTER_TILE);
      if ((long long)(box.z - box.x + 1) * (box.w - box.y + 1) <= RASTER_SMALL) {
        for (int ty = box.y; ty <= box.w; ++ty)
          for (int tx = box.x; tx <= box.z; ++tx) atomicAdd(tile_count + (size_t)ty * ntx + tx, 1);
      } else {
        large_list[atomicAdd(large_count, 1)] = (int)f;
      }
    }
  }
  fbox[f] = box;
}

// One workgroup: start[i] = sum of count[0 .. i), start[nt] = the total; count[i] becomes the fill cursor of tile i (= start[i]).
// Each thread owns a contiguous run of tiles; the 256 run sums are scanned in LDS.
__global__ void __launch_bounds__(256) raster_scan_kernel(int* __restrict__ count, int nt, int* __restrict__ start) {
  __shared__ int s[256];
  const int t = threadIdx.x, per = (nt + 255) / 256;
  const long long b0 = (long long)t * per;
  const int b = (int)(b0 < nt ? b0 : nt), e = (int)(b0 + per < nt ? b0 + per : nt);
  int sum = 0;
  for (int i = b; i < e; ++i) sum += count[i];
  s[t] = sum;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int v = t >= off ? s[t - off] : 0;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  int run = s[t] - sum;
  for (int i = b; i < e; ++i) { const int c = count[i]; start[i] = run; count[i] = run; run += c; }
  if (t == 255) start[nt] = s[255];
}

__global__ void __launch_bounds__(256) raster_fill_kernel(long long F, const int4* __restrict__ fbox, int ntx, int* __restrict__ cursor,
                                                          int* __restrict__ bin_tris) {
  const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const int4 box = fbox[f];
  if (box.z < box.x || (long long)(box.z - box.x + 1) * (box.w - box.y + 1) > RASTER_SMALL) return;
  for (int ty = box.y; ty <= box.w; ++ty)
    for (int tx = box.x; tx <= box.z; ++tx) bin_tris[atomicAdd(cursor + (size_t)ty * ntx + tx, 1)] = (int)f;
}

// A face as the pixel loop reads it.  e[k] = (Px, Py, dx, dy, s, tie) of edge k (0: AB, 1: BC, 2: CA): the edge function at (x, y) is
// (dx * (y - Py) - dy * (x - Px)) * s, >= 0 inside.  (P, dx, dy) run from the lexicographically smaller end point to the larger one and
// s = +-1 carries the edge's own direction and the face's orientation, so the two faces of a shared edge evaluate the SAME rounded
// expression with opposite signs: a sample is inside exactly one of them whatever the rounding.  tie: the top-left rule of grid.hip's
// voxel_columns_kernel on the oriented edge (a sample exactly on the edge belongs to the face iff tie != 0).
struct __attribute__((aligned(16))) RasterTri { double e[3][6]; double w[3]; int id, live; };

__device__ __forceinline__ void raster_edge(const double* P, const double* Q, double sgn, double* e) {
  const double dxo = (Q[0] - P[0]) * sgn, dyo = (Q[1] - P[1]) * sgn;
  const bool swap = Q[0] < P[0] || (Q[0] == P[0] && Q[1] < P[1]);
  const double* p = swap ? Q : P, *q = swap ? P : Q;
  e[0] = p[0]; e[1] = p[1]; e[2] = q[0] - p[0]; e[3] = q[1] - p[1];
  e[4] = swap ? -sgn : sgn;
  e[5] = (dyo > 0.0 || (dyo == 0.0 && dxo < 0.0)) ? 1.0 : 0.0;
}

// The hot path.  One workgroup per tile, one lane per pixel; the tile's faces pass through LDS RASTER_TB at a time (every lane reads the
// same staged face: broadcast reads), first the tile's own list, then the faces too large to bin (those are tested against the tile
// when staged).  Lanes past W or H take part in the staging and the barriers and neither test nor store.
__global__ void __launch_bounds__(256) raster_tile_kernel(const int* __restrict__ faces, const double* __restrict__ proj, const int4* __restrict__ fbox,
                                                          const int* __restrict__ tile_start, const int* __restrict__ bin_tris,
                                                          const int* __restrict__ large_count, const int* __restrict__ large_list, int H, int W,
                                                          int ntx, double pc, double znear, double zfar, float* __restrict__ depth,
                                                          int* __restrict__ tri, int* __restrict__ hits) {
  __shared__ RasterTri st[RASTER_TB];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int tile = blockIdx.x, tx = tile % ntx, ty = tile / ntx;
  const int col = tx * RASTER_TILE + (wave & 1) * 8 + (lane & 7), row = ty * RASTER_TILE + (wave >> 1) * 8 + (lane >> 3);
  const bool active = col < W && row < H;
  const double px = (double)col + pc, py = (double)row + pc;
  double best = INFINITY;
  int best_tri = -1, nhits = 0;
  for (int phase = 0; phase < 2; ++phase) {
    const int* list = phase == 0 ? bin_tris + tile_start[tile] : large_list;
    const int n = phase == 0 ? tile_start[tile + 1] - tile_start[tile] : *large_count;
    for (int base = 0; base < n; base += RASTER_TB) {
      const int nb = n - base < RASTER_TB ? n - base : RASTER_TB;
      if (t < nb) {
        const int f = list[base + t];
        int live = 1;
        if (phase == 1) { const int4 box = fbox[f]; live = box.x <= tx && tx <= box.z && box.y <= ty && ty <= box.w; }
        if (live) {
          const double* A = proj + 3 * (long long)faces[3 * (long long)f], *B = proj + 3 * (long long)faces[3 * (long long)f + 1],
                       *C = proj + 3 * (long long)faces[3 * (long long)f + 2];
          const double area = (B[0] - A[0]) * (C[1] - A[1]) - (B[1] - A[1]) * (C[0] - A[0]);
          if (area > 0.0 || area < 0.0) {                               // zero (and NaN) area covers nothing
            const double sgn = area > 0.0 ? 1.0 : -1.0;
            raster_edge(A, B, sgn, st[t].e[0]); raster_edge(B, C, sgn, st[t].e[1]); raster_edge(C, A, sgn, st[t].e[2]);
            st[t].w[0] = A[2]; st[t].w[1] = B[2]; st[t].w[2] = C[2];
          } else {
            live = 0;
          }
        }
        st[t].id = f; st[t].live = live;
      }
      __syncthreads();
      if (active) {
        for (int j = 0; j < nb; ++j) {
          const RasterTri& s = st[j];
          if (!s.live) continue;
          const double eab = (s.e[0][2] * (py - s.e[0][1]) - s.e[0][3] * (px - s.e[0][0])) * s.e[0][4];
          if (!(eab > 0.0 || (eab == 0.0 && s.e[0][5] != 0.0))) continue;
          const double ebc = (s.e[1][2] * (py - s.e[1][1]) - s.e[1][3] * (px - s.e[1][0])) * s.e[1][4];
          if (!(ebc > 0.0 || (ebc == 0.0 && s.e[1][5] != 0.0))) continue;
          const double eca = (s.e[2][2] * (py - s.e[2][1]) - s.e[2][3] * (px - s.e[2][0])) * s.e[2][4];
          if (!(eca > 0.0 || (eca == 0.0 && s.e[2][5] != 0.0))) continue;
          const double esum = (eab + ebc) + eca;
          if (!(esum > 0.0)) continue;
          const double d = esum / ((ebc * s.w[0] + eca * s.w[1]) + eab * s.w[2]);       // 1 / depth is linear in the weights
          if (!(znear < d && d < zfar)) continue;
          ++nhits;
          if (d < best || (d == best && s.id < best_tri)) { best = d; best_tri = s.id; }
        }
      }
      __syncthreads();
    }
  }
  if (!active) return;
  const size_t o = (size_t)row * W + col;
  depth[o] = nhits ? (float)best : 0.0f;
  if (tri) tri[o] = best_tri;
  if (hits) hits[o] = nhits;
}

// ---- the box dilation of render_mask.py:92-93, rows then columns, and cv2.boundingRect of the result ---------------------------------
__global__ void __launch_bounds__(256) dilate_rows_kernel(const uint8_t* __restrict__ mask, int H, int W, int ax, uint8_t* __restrict__ tmp) {
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long long)H * W) return;
  const int c = (int)(id % W);
  const uint8_t* line = mask + (id - c);
  const int c0 = c - ax > 0 ? c - ax : 0, c1 = c + ax < W - 1 ? c + ax : W - 1;
  int any = 0;
  for (int k = c0; k <= c1; ++k) any |= line[k] > 0;
  tmp[id] = (uint8_t)any;
}

struct RectAcc { int x0, y0, x1, y1; };                     // smallest / largest set column and row; x1 = -1: nothing set
__device__ __forceinline__ RectAcc rect_join(RectAcc a, RectAcc b) {
  return RectAcc{a.x0 < b.x0 ? a.x0 : b.x0, a.y0 < b.y0 ? a.y0 : b.y0, a.x1 > b.x1 ? a.x1 : b.x1, a.y1 > b.y1 ? a.y1 : b.y1};
}
__device__ __forceinline__ RectAcc rect_block(RectAcc mine, RectAcc* s) {      // tree over the 256 threads, in index order
  const int t = threadIdx.x;
  s[t] = mine;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (t < off) s[t] = rect_join(s[t], s[t + off]);
    __syncthreads();
  }
  return s[0];
}

__global__ void __launch_bounds__(256) dilate_cols_kernel(const uint8_t* __restrict__ tmp, int H, int W, int ay, uint8_t* __restrict__ out,
                                                          RectAcc* __restrict__ partial) {
  __shared__ RectAcc s[256];
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  RectAcc mine{0x7fffffff, 0x7fffffff, -1, -1};
  if (id < (long long)H * W) {
    const int c = (int)(id % W), r = (int)(id / W);
    const int r0 = r - ay > 0 ? r - ay : 0, r1 = r + ay < H - 1 ? r + ay : H - 1;
    int any = 0;
    for (int k = r0; k <= r1; ++k) any |= tmp[(size_t)k * W + c];
    out[id] = any ? 255 : 0;
    if (any) mine = RectAcc{c, r, c, r};
  }
  const RectAcc all = rect_block(mine, s);
  if (threadIdx.x == 0) partial[blockIdx.x] = all;
}

__global__ void __launch_bounds__(256) dilate_rect_kernel(const RectAcc* __restrict__ partial, long long n, int* __restrict__ bbox) {
  __shared__ RectAcc s[256];
  RectAcc mine{0x7fffffff, 0x7fffffff, -1, -1};
  for (long long i = threadIdx.x; i < n; i += 256) mine = rect_join(mine, partial[i]);
  const RectAcc all = rect_block(mine, s);
  if (threadIdx.x == 0) {
    const bool any = all.x1 >= 0;
    bbox[0] = any ? all.x0 : 0; bbox[1] = any ? all.y0 : 0; bbox[2] = any ? all.x1 - all.x0 + 1 : 0; bbox[3] = any ? all.y1 - all.y0 + 1 : 0;
  }
}

static bool raster_shape(int64_t V, int64_t F, int32_t H, int32_t W) {
  return V >= 0 && V < (1LL << 31) && F >= 0 && F < (1LL << 29) && H >= 1 && W >= 1 && (int64_t)H * W < (1LL << 31);
}
static const char* const RASTER_SHAPE_MSG = "need 0 <= num_verts < 2^31, 0 <= num_faces < 2^29, height, width >= 1, height * width < 2^31";

struct RasterWs { size_t proj, fbox, tile_start, tile_cursor, bin_tris, large_count, large_list, total; long long nt; int ntx; };
static RasterWs raster_workspace(int64_t V, int64_t F, int32_t H, int32_t W) {
  RasterWs w;
  w.ntx = (W + RASTER_TILE - 1) / RASTER_TILE;
  w.nt = (long long)w.ntx * ((H + RASTER_TILE - 1) / RASTER_TILE);
  size_t o = 0;
  w.proj = o; o += up16((size_t)V * 3 * sizeof(double));
  w.fbox = o; o += up16((size_t)F * sizeof(int4));
  w.tile_start = o; o += up16((size_t)(w.nt + 1) * sizeof(int));
  w.tile_cursor = o; o += up16((size_t)w.nt * sizeof(int));
  w.bin_tris = o; o += up16((size_t)F * RASTER_SMALL * sizeof(int));
  w.large_count = o; o += 16;
  w.large_list = o; o += up16((size_t)F * sizeof(int));
  w.total = o;
  return w;
}

// The camera of rnerf_generate_rays' arguments; false when the rotation has no finite inverse.  The inverse is the adjugate over the
// determinant, every operation rounded (the build has -ffp-contract=off), as tests/helpers/mesh_raster_ref.py restates it.
static bool raster_camera(const float* camtoworld, int opencv, double fx, double fy, double cx, double cy, double pc, RasterCam* out) {
  double r[3][3], k[3][3];
  for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) r[i][j] = (double)camtoworld[4 * i + j]; out->t[i] = (double)camtoworld[4 * i + 3]; }
  for (int i = 0; i < 3; ++i)                               // k[i][j]: the cofactor of r[i][j]
    for (int j = 0; j < 3; ++j) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      k[i][j] = r[i1][j1] * r[i2][j2] - r[i1][j2] * r[i2][j1];
    }
  const double det = (r[0][0] * k[0][0] + r[0][1] * k[0][1]) + r[0][2] * k[0][2];
  if (!(isfinite(det) && det != 0.0)) return false;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      out->ri[3 * i + j] = k[j][i] / det;
      if (!isfinite(out->ri[3 * i + j])) return false;
    }
  out->fx = (double)(float)fx; out->fy = (double)(float)fy; out->cx = (double)(float)cx; out->cy = (double)(float)cy; out->pc = (double)(float)pc;
  out->sy = opencv ? 1.0 : -1.0; out->sz = opencv ? 1.0 : -1.0;
  return true;
}

static bool dilate_shape(int32_t H, int32_t W) { return H >= 1 && W >= 1 && (int64_t)H * W < (1LL << 31); }

}  // namespace rnerf

using namespace rnerf;

extern "C" size_t rnerf_mesh_depth_workspace_bytes(int64_t num_verts, int64_t num_faces, int32_t height, int32_t width) {
  if (!raster_shape(num_verts, num_faces, height, width)) {
    set_error("rnerf_mesh_depth_workspace_bytes: %s", RASTER_SHAPE_MSG);
    return 0;
  }
  return raster_workspace(num_verts, num_faces, height, width).total;
}

extern "C" int rnerf_mesh_depth(const double* verts, int64_t num_verts, const int32_t* faces, int64_t num_faces, const float* camtoworld,
                                int32_t opencv, double fx, double fy, double cx, double cy, double pixel_center, int32_t height, int32_t width,
                                double znear, double zfar, float* depth, int32_t* tri, int32_t* hits, int64_t* skipped, void* workspace,
                                void* stream) {
  RNERF_CHECK_ARG(camtoworld && depth && skipped, "rnerf_mesh_depth: null pointer (camtoworld, depth, skipped)");
  RNERF_CHECK_ARG(raster_shape(num_verts, num_faces, height, width), "rnerf_mesh_depth: %s", RASTER_SHAPE_MSG);
  RNERF_CHECK_ARG(num_faces == 0 || (verts && faces && workspace && num_verts > 0),
                  "rnerf_mesh_depth: null pointer (verts, faces, workspace) or num_verts == 0 with num_faces > 0");
  RNERF_CHECK_ARG(opencv == 0 || opencv == 1, "rnerf_mesh_depth: opencv must be 0 or 1");
  RNERF_CHECK_ARG(isfinite(fx) && isfinite(fy) && fx != 0.0 && fy != 0.0 && isfinite(cx) && isfinite(cy) && isfinite(pixel_center),
                  "rnerf_mesh_depth: fx, fy must be finite and non-zero, cx, cy, pixel_center finite");
  RNERF_CHECK_ARG(znear < zfar, "rnerf_mesh_depth: need znear < zfar");
  RNERF_CHECK_ARG(((uintptr_t)verts & 7) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)skipped & 7) == 0,
                  "rnerf_mesh_depth: verts and skipped must be 8-byte, workspace 16-byte aligned");
  RasterCam c;
  RNERF_CHECK_ARG(raster_camera(camtoworld, opencv, fx, fy, cx, cy, pixel_center, &c), "rnerf_mesh_depth: the rotation of camtoworld has no finite inverse");
  hipStream_t st = (hipStream_t)stream;
  const size_t npix = (size_t)height * width;
  RNERF_CHECK_HIP(hipMemsetAsync(skipped, 0, sizeof(int64_t), st));
  if (num_faces == 0) {                                            // the empty image; nothing below indexes the mesh
    RNERF_CHECK_HIP(hipMemsetAsync(depth, 0, npix * sizeof(float), st));
    if (tri) RNERF_CHECK_HIP(hipMemsetAsync(tri, 0xFF, npix * sizeof(int32_t), st));
    if (hits) RNERF_CHECK_HIP(hipMemsetAsync(hits, 0, npix * sizeof(int32_t), st));
    return RNERF_OK;
  }
  const RasterWs w = raster_workspace(num_verts, num_faces, height, width);
  char* ws = (char*)workspace;
  double* proj = (double*)(ws + w.proj);
  int4* fbox = (int4*)(ws + w.fbox);
  int* tile_start = (int*)(ws + w.tile_start), *tile_cursor = (int*)(ws + w.tile_cursor), *bin_tris = (int*)(ws + w.bin_tris);
  int* large_count = (int*)(ws + w.large_count), *large_list = (int*)(ws + w.large_list);
  RNERF_CHECK_HIP(hipMemsetAsync(tile_cursor, 0, (size_t)w.nt * sizeof(int), st));
  RNERF_CHECK_HIP(hipMemsetAsync(large_count, 0, 16, st));
  const unsigned fblocks = (unsigned)((num_faces + 255) / 256);
  hipLaunchKernelGGL(raster_project_kernel, dim3((unsigned)((num_verts + 255) / 256)), dim3(256), 0, st, verts, (long long)num_verts, c, proj);
  hipLaunchKernelGGL(raster_face_kernel, dim3(fblocks), dim3(256), 0, st, faces, (long long)num_faces, proj, height, width, w.ntx, c.pc, fbox,
                     tile_cursor, large_count, large_list, (unsigned long long*)skipped);
  hipLaunchKernelGGL(raster_scan_kernel, dim3(1), dim3(256), 0, st, tile_cursor, (int)w.nt, tile_start);
  hipLaunchKernelGGL(raster_fill_kernel, dim3(fblocks), dim3(256), 0, st, (long long)num_faces, fbox, w.ntx, tile_cursor, bin_tris);
  hipLaunchKernelGGL(raster_tile_kernel, dim3((unsigned)w.nt), dim3(256), 0, st, faces, proj, fbox, tile_start, bin_tris, large_count, large_list,
                     height, width, w.ntx, c.pc, znear, zfar, depth, tri, hits);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" size_t rnerf_mask_dilate_workspace_bytes(int32_t height, int32_t width) {
  if (!dilate_shape(height, width)) {
    set_error("rnerf_mask_dilate_workspace_bytes: need height, width >= 1, height * width < 2^31");
    return 0;
  }
  const size_t npix = (size_t)height * width;
  return up16(npix) + ((npix + 255) / 256) * sizeof(RectAcc);
}

extern "C" int rnerf_mask_dilate(const uint8_t* mask, int32_t height, int32_t width, int32_t ky, int32_t kx, uint8_t* out, int32_t* bbox,
                                 void* workspace, void* stream) {
  RNERF_CHECK_ARG(mask && out && workspace, "rnerf_mask_dilate: null pointer");
  RNERF_CHECK_ARG(dilate_shape(height, width), "rnerf_mask_dilate: need height, width >= 1, height * width < 2^31");
  RNERF_CHECK_ARG(ky >= 1 && kx >= 1 && (ky & 1) && (kx & 1), "rnerf_mask_dilate: ky and kx must be odd and >= 1");
  const size_t npix = (size_t)height * width;
  RNERF_CHECK_ARG(out + npix <= mask || mask + npix <= out, "rnerf_mask_dilate: out may not alias mask");
  RNERF_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)bbox & 3) == 0, "rnerf_mask_dilate: workspace must be 16-byte, bbox 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  uint8_t* tmp = (uint8_t*)workspace;
  RectAcc* partial = (RectAcc*)((char*)workspace + up16(npix));
  const long long blocks = (long long)((npix + 255) / 256);
  hipLaunchKernelGGL(dilate_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, st, mask, height, width, kx / 2, tmp);
  hipLaunchKernelGGL(dilate_cols_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const uint8_t*)tmp, height, width, ky / 2, out, partial);
  if (bbox) hipLaunchKernelGGL(dilate_rect_kernel, dim3(1), dim3(256), 0, st, (const RectAcc*)partial, blocks, bbox);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}
