// Marching cubes on the device: the triangle mesh of an iso-surface of a voxel grid that is already there.
// Reference: mcubes.marching_cubes at voxelize_mesh.py:122-135 (the voxelised grid's preview OBJ), calib/make_visual_hull.py:148-157 (the
// carved hull's) and extract_mesh.py:232-268 (a trained field's density).  PyMCubes' tie rule, vertex order and per-case triangulation
// are not reproduced; the mesh is the one include/rnerf.h specifies: one vertex per crossed grid edge in node-linear
// order, triangles in cell-linear order from the generated table mc_tables.h, counter-clockwise seen from the empty side.
//
// A workgroup of four waves owns a brick of 1024 consecutive nodes of the flattened [Gx][Gy][Gz] field (z fastest, so a wave reads 64
// consecutive floats of a row); a wave takes four 64-node chunks of it one after the other.  Consecutive bricks are consecutive in the
// output order, so the position of everything a brick emits is the exclusive sum of the counts of the bricks before it (one
// single-workgroup scan) plus a prefix inside the brick (ballots inside a chunk, LDS across chunks).  No atomics, no workgroup waits on
// another: the same bytes on every run.
#include "common.h"
#include "mc_tables.h"

#include <math.h>
#include <string.h>

namespace rnerf {

constexpr int MC_CHUNKS = 4;                              // chunks of 64 nodes per wave
constexpr int MC_BRICK = 256 * MC_CHUNKS;                 // nodes per workgroup
constexpr long long MC_MAX_NODES = ((1LL << 31) - 1) / 3; // 3 N <= 2^31 - 1: vertex indices fit int32 (and 5 N, the triangles, uint32)

static const int8_t mc_tri_host[256][16] = RNERF_MC_TRI;
__constant__ int8_t mc_tri[256][16] = RNERF_MC_TRI;
__constant__ int8_t mc_ntri[256] = RNERF_MC_NTRI;

struct McGrid { int gx, gy, gz, n; };                     // n = gx gy gz

struct McNode { int i, j, k; bool hx, hy, hz; };          // a node's coordinates and whether it has a neighbour one up on each axis
__device__ __forceinline__ McNode mc_node(const McGrid& g, int n) {
  McNode p;
  p.k = n % g.gz;
  const int r = n / g.gz;
  p.j = r % g.gy;
  p.i = r / g.gy;
  p.hx = p.i + 1 < g.gx; p.hy = p.j + 1 < g.gy; p.hz = p.k + 1 < g.gz;
  return p;
}

__device__ __forceinline__ bool mc_solid(float f, double iso) { return (double)f > iso; }      // NaN is empty

// Bits 0..2: the node's x-, y-, z-edge is crossed.  `n` must be a node of the grid.
__device__ __forceinline__ int mc_owned(const float* __restrict__ field, const McGrid& g, int n, const McNode& p, double iso) {
  const bool s0 = mc_solid(field[n], iso);
  int m = 0;
  if (p.hx && mc_solid(field[n + g.gy * g.gz], iso) != s0) m |= 1;
  if (p.hy && mc_solid(field[n + g.gz], iso) != s0) m |= 2;
  if (p.hz && mc_solid(field[n + 1], iso) != s0) m |= 4;
  return m;
}

// The case of the cell whose lowest corner is node n: bit x + 2y + 4z.  0 where the node has no cell.
__device__ __forceinline__ int mc_case(const float* __restrict__ field, const McGrid& g, int n, const McNode& p, double iso) {
  if (!(p.hx && p.hy && p.hz)) return 0;
  const int sx = g.gy * g.gz, sy = g.gz;
  int c = 0;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const float f = field[n + (m & 1) * sx + ((m >> 1) & 1) * sy + (m >> 2)];
    c |= (int)mc_solid(f, iso) << m;
  }
  return c;
}

__device__ __forceinline__ int mc_popc_below(unsigned long long b, int lane) { return __popcll(b & ((1ULL << lane) - 1ULL)); }

// Exclusive prefix, over the nodes of a brick in order, of a per-node count in 0..7, for a wave's MC_CHUNKS chunks.  cnt[c] is the
// count of this lane's node in the wave's chunk c (0 for a node past the grid); on return pre[c] is the sum over the brick's nodes
// before it.  Returns the brick's total.  `lds` holds 4 ints; all four waves must call this together.
__device__ __forceinline__ int mc_brick_prefix(const int (&cnt)[MC_CHUNKS], int (&pre)[MC_CHUNKS], int* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int run = 0;
#pragma unroll
  for (int c = 0; c < MC_CHUNKS; ++c) {
    const unsigned long long b0 = __ballot(cnt[c] & 1), b1 = __ballot(cnt[c] & 2), b2 = __ballot(cnt[c] & 4);
    pre[c] = run + mc_popc_below(b0, lane) + 2 * mc_popc_below(b1, lane) + 4 * mc_popc_below(b2, lane);
    run += __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
  }
  __syncthreads();                                       // a previous use of lds is over
  if (lane == 0) lds[wave] = run;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int v = lds[w];
    if (w < wave) before += v;
    total += v;
  }
#pragma unroll
  for (int c = 0; c < MC_CHUNKS; ++c) pre[c] += before;
  return total;
}

__device__ __forceinline__ int mc_chunk_node(int c) {     // the node of this lane in chunk c of its wave
  return blockIdx.x * MC_BRICK + ((threadIdx.x >> 6) * MC_CHUNKS + c) * 64 + (threadIdx.x & 63);
}

// Launch 1: counts[brick] = {vertices, triangles} the brick's nodes and cells give.
__global__ void __launch_bounds__(256) mc_count_kernel(const float* __restrict__ field, McGrid g, double iso, uint2* __restrict__ counts) {
  __shared__ int lds[8];
  int nv[MC_CHUNKS], nt[MC_CHUNKS], pre[MC_CHUNKS];
#pragma unroll
  for (int c = 0; c < MC_CHUNKS; ++c) {
    const int n = mc_chunk_node(c);
    nv[c] = nt[c] = 0;
    if (n < g.n) {
      const McNode p = mc_node(g, n);
      nv[c] = __popc(mc_owned(field, g, n, p, iso));
      nt[c] = mc_ntri[mc_case(field, g, n, p, iso)];
    }
  }
  const int tv = mc_brick_prefix(nv, pre, lds), tt = mc_brick_prefix(nt, pre, lds + 4);
  if (threadIdx.x == 0) counts[blockIdx.x] = make_uint2((unsigned)tv, (unsigned)tt);
}

// Launch 2: one workgroup turns the brick counts into exclusive offsets in place, 8192 bricks per pass in brick order (a thread takes 8
// consecutive bricks, so a pass costs one round of loads and two barriers), and writes the totals.  Offsets are modulo 2^32 (the size
// limit keeps them below it); the totals are summed in 64 bits.
constexpr int MC_SCAN_ITEMS = 8;
__global__ void __launch_bounds__(1024) mc_scan_kernel(uint2* __restrict__ counts, int nbricks, long long* __restrict__ totals) {
  __shared__ unsigned wsum[2][16];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  unsigned long long carry_v = 0, carry_t = 0;
  for (int base = 0; base < nbricks; base += 1024 * MC_SCAN_ITEMS) {
    const int first = base + t * MC_SCAN_ITEMS;
    uint2 own[MC_SCAN_ITEMS];
    unsigned sv = 0, sf = 0;
#pragma unroll
    for (int i = 0; i < MC_SCAN_ITEMS; ++i) own[i] = first + i < nbricks ? counts[first + i] : make_uint2(0u, 0u);
#pragma unroll
    for (int i = 0; i < MC_SCAN_ITEMS; ++i) {             // exclusive inside the thread
      const uint2 c = own[i];
      own[i] = make_uint2(sv, sf);
      sv += c.x; sf += c.y;
    }
    unsigned v = sv, f = sf;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {                    // inclusive scan of the threads' sums inside the wave
      const unsigned pv = __shfl_up(v, d), pf = __shfl_up(f, d);
      if (lane >= d) { v += pv; f += pf; }
    }
    __syncthreads();                                     // the previous pass has read wsum
    if (lane == 63) { wsum[0][wave] = v; wsum[1][wave] = f; }
    __syncthreads();
    unsigned before_v = 0, before_f = 0, tot_v = 0, tot_f = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      const unsigned a = wsum[0][w], b = wsum[1][w];
      if (w < wave) { before_v += a; before_f += b; }
      tot_v += a; tot_f += b;
    }
    const unsigned tv = (unsigned)carry_v + before_v + v - sv, tf = (unsigned)carry_t + before_f + f - sf;
#pragma unroll
    for (int i = 0; i < MC_SCAN_ITEMS; ++i)
      if (first + i < nbricks) counts[first + i] = make_uint2(tv + own[i].x, tf + own[i].y);
    carry_v += tot_v; carry_t += tot_f;
  }
  if (t == 0) { totals[0] = (long long)carry_v; totals[1] = (long long)carry_t; }
}

// Launch 3: vbase[node] = the index of the node's first vertex; the node's 0..3 vertices, x-, y-, z-edge in turn.  Position: the node's
// index, plus t = (iso - f1) / (f2 - f1) on the edge's axis in float64 (individually rounded: -ffp-contract=off), f1 the node's value;
// t = 0.5 where that is not in [0, 1] (a non-finite or NaN endpoint), so every vertex is finite and on its edge.
__global__ void __launch_bounds__(256) mc_vertex_kernel(const float* __restrict__ field, McGrid g, double iso, const uint2* __restrict__ offsets,
                                                        int* __restrict__ vbase, double* __restrict__ verts, long long capacity,
                                                        int* __restrict__ overflow) {
  __shared__ int lds[4];
  int own[MC_CHUNKS], nv[MC_CHUNKS], pre[MC_CHUNKS];
#pragma unroll
  for (int c = 0; c < MC_CHUNKS; ++c) {
    const int n = mc_chunk_node(c);
    own[c] = n < g.n ? mc_owned(field, g, n, mc_node(g, n), iso) : 0;
    nv[c] = __popc(own[c]);
  }
  mc_brick_prefix(nv, pre, lds);
  const unsigned brick_base = offsets[blockIdx.x].x;
#pragma unroll
  for (int c = 0; c < MC_CHUNKS; ++c) {
    const int n = mc_chunk_node(c);
    if (n >= g.n) continue;
    long long v = (long long)(brick_base + (unsigned)pre[c]);
    vbase[n] = (int)v;
    if (own[c] == 0) continue;
    const McNode p = mc_node(g, n);
    const double f1 = (double)field[n];
    const int stride[3] = {g.gy * g.gz, g.gz, 1};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!(own[c] & (1 << a))) continue;
      const double f2 = (double)field[n + stride[a]];
      double t = (iso - f1) / (f2 - f1);
      if (!(t >= 0.0 && t <= 1.0)) t = 0.5;
      if (v < capacity) {
        verts[v * 3 + 0] = (double)p.i + (a == 0 ? t : 0.0);
        verts[v * 3 + 1] = (double)p.j + (a == 1 ? t : 0.0);
        verts[v * 3 + 2] = (double)p.k + (a == 2 ? t : 0.0);
      } else {
        *overflow = 1;
      }
      ++v;
    }
  }
}

// Launch 4: the triangles of every cell, in cell order and within a cell in the table's order.  A table entry is an edge id
// 4 axis + a + 2 b; the edge belongs to the node at the cell's corner (a, b) on the two other axes, and its vertex is
// vbase[that node] + the number of crossed edges of lower axis at that node (from the owner's field values; it may lie in another brick,
// which is why this is a launch of its own).
__global__ void __launch_bounds__(256) mc_triangle_kernel(const float* __restrict__ field, McGrid g, double iso, const uint2* __restrict__ offsets,
                                                          const int* __restrict__ vbase, int* __restrict__ faces, long long capacity,
                                                          int* __restrict__ overflow) {
  __shared__ int lds[4];
  int cs[MC_CHUNKS], nt[MC_CHUNKS], pre[MC_CHUNKS];
#pragma unroll
  for (int c = 0; c < MC_CHUNKS; ++c) {
    const int n = mc_chunk_node(c);
    cs[c] = n < g.n ? mc_case(field, g, n, mc_node(g, n), iso) : 0;
    nt[c] = mc_ntri[cs[c]];
  }
  mc_brick_prefix(nt, pre, lds);
  const unsigned brick_base = offsets[blockIdx.x].y;
  const int sx = g.gy * g.gz, sy = g.gz;
#pragma unroll
  for (int c = 0; c < MC_CHUNKS; ++c) {
    if (nt[c] == 0) continue;
    const int n = mc_chunk_node(c);
    const long long f0 = (long long)(brick_base + (unsigned)pre[c]);
    for (int e = 0; e < 3 * nt[c]; ++e) {
      const int id = mc_tri[cs[c]][e], axis = id >> 2, a = id & 1, b = (id >> 1) & 1;
      // the owner's offset from the cell's lowest corner: (a, b) on the two other axes, the lower axis first
      const int ox = axis == 0 ? 0 : a, oy = axis == 0 ? a : (axis == 1 ? 0 : b), oz = axis == 2 ? 0 : b;
      const int owner = n + ox * sx + oy * sy + oz;
      int v = vbase[owner];
      if (axis > 0) {
        const int m = mc_owned(field, g, owner, mc_node(g, owner), iso);
        v += (m & 1) + (axis == 2 ? (m >> 1) & 1 : 0);
      }
      const long long slot = f0 + e / 3;
      if (slot < capacity) faces[slot * 3 + e % 3] = v;
      else *overflow = 1;
    }
  }
}

static const char* const MC_DIMS_MSG = "need dims >= 2 and 3 * dims[0] * dims[1] * dims[2] <= 2^31 - 1";
static bool mc_grid(const int32_t* dims, McGrid* out) {
  if (!dims || dims[0] < 2 || dims[1] < 2 || dims[2] < 2) return false;
  const long long xy = (long long)dims[0] * dims[1];
  if (xy > MC_MAX_NODES || xy * dims[2] > MC_MAX_NODES) return false;
  out->gx = dims[0]; out->gy = dims[1]; out->gz = dims[2]; out->n = (int)(xy * dims[2]);
  return true;
}
static int mc_bricks(const McGrid& g) { return (g.n + MC_BRICK - 1) / MC_BRICK; }

}  // namespace rnerf

using namespace rnerf;

extern "C" int rnerf_marching_cubes_table(int8_t* tri_out) {
  RNERF_CHECK_ARG(tri_out, "rnerf_marching_cubes_table: null pointer");
  memcpy(tri_out, mc_tri_host, sizeof(mc_tri_host));
  return RNERF_OK;
}

extern "C" size_t rnerf_marching_cubes_workspace_bytes(const int32_t dims[3]) {
  McGrid g;
  if (!mc_grid(dims, &g)) {
    set_error("rnerf_marching_cubes_workspace_bytes: %s", MC_DIMS_MSG);
    return 0;
  }
  return (size_t)mc_bricks(g) * sizeof(uint2) + (size_t)g.n * sizeof(int32_t);
}

extern "C" int rnerf_marching_cubes_count(const float* field, const int32_t dims[3], double iso, void* workspace, int64_t* totals,
                                          void* stream) {
  RNERF_CHECK_ARG(field && dims && workspace && totals, "rnerf_marching_cubes_count: null pointer");
  McGrid g;
  RNERF_CHECK_ARG(mc_grid(dims, &g), "rnerf_marching_cubes_count: %s", MC_DIMS_MSG);
  RNERF_CHECK_ARG(isfinite(iso), "rnerf_marching_cubes_count: iso must be finite");
  RNERF_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)totals & 7) == 0 && ((uintptr_t)field & 3) == 0,
                  "rnerf_marching_cubes_count: workspace and totals must be 8-byte, field 4-byte aligned");
  const int nb = mc_bricks(g);
  hipLaunchKernelGGL(mc_count_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, field, g, iso, (uint2*)workspace);
  RNERF_CHECK_LAUNCH();
  hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (uint2*)workspace, nb, (long long*)totals);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_marching_cubes_emit(const float* field, const int32_t dims[3], double iso, const void* workspace, double* verts,
                                         int64_t verts_capacity, int32_t* faces, int64_t faces_capacity, int32_t* overflow, void* stream) {
  RNERF_CHECK_ARG(field && dims && workspace && overflow, "rnerf_marching_cubes_emit: null pointer");
  RNERF_CHECK_ARG(verts_capacity >= 0 && faces_capacity >= 0, "rnerf_marching_cubes_emit: negative capacity");
  RNERF_CHECK_ARG((verts || verts_capacity == 0) && (faces || faces_capacity == 0), "rnerf_marching_cubes_emit: null pointer with a capacity above 0");
  McGrid g;
  RNERF_CHECK_ARG(mc_grid(dims, &g), "rnerf_marching_cubes_emit: %s", MC_DIMS_MSG);
  RNERF_CHECK_ARG(isfinite(iso), "rnerf_marching_cubes_emit: iso must be finite");
  RNERF_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)verts & 7) == 0 && (((uintptr_t)field | (uintptr_t)faces | (uintptr_t)overflow) & 3) == 0,
                  "rnerf_marching_cubes_emit: workspace and verts must be 8-byte, field, faces and overflow 4-byte aligned");
  RNERF_CHECK_HIP(hipMemsetAsync(overflow, 0, sizeof(int32_t), (hipStream_t)stream));
  const int nb = mc_bricks(g);
  const uint2* offsets = (const uint2*)workspace;
  int* vbase = (int*)((uint2*)workspace + nb);            // the vertex launch's output; what _count left, the brick offsets, is only read
  if (verts_capacity > 0) {                               // (a call for triangles alone reads the vbase an earlier call left)
    hipLaunchKernelGGL(mc_vertex_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, field, g, iso, offsets, vbase, verts, (long long)verts_capacity,
                       overflow);
    RNERF_CHECK_LAUNCH();
  }
  if (faces_capacity > 0) {
    hipLaunchKernelGGL(mc_triangle_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, field, g, iso, offsets, (const int*)vbase, faces,
                       (long long)faces_capacity, overflow);
    RNERF_CHECK_LAUNCH();
  }
  return RNERF_OK;
}
