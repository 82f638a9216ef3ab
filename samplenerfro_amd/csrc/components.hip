// 3-D connected components of a voxel grid: the labelling, per-component statistics and the rewrite of a grid from a keep table that
// visual_hull.clean / voxelize.clean / extract.extract_mesh use to drop floaters and fill cavities (samplenerfro_amd/components.py).
// The reference has no code for this: its README sends the user to Blender ("remove the noisy components in the proxy geometry").
//
// Grids are [X][Y][Z], z fastest, linear index x*Y*Z + y*Z + z < 2^31.  The label of a voxel of the labelled phase is the smallest linear
// index of its component, every other voxel is -1: a pure function of the input, so the bytes are the same on every run although the
// union-find below hooks with atomics in whatever order the hardware takes.
//
// Union-find with min-hooking: parent[i] <= i always, a root is parent[r] == r, and uniting hooks the larger root under the smaller with
// atomicMin.  A root is therefore the minimum of its tree, and once every adjacent pair is united the root is the component's minimum.
// Three launches, whatever the grid holds:
//   1. cc_tile_kernel: one workgroup unites an 8 x 8 x 64 tile in LDS and stores every voxel's tile-local root as a global index.
//   2. cc_merge_kernel: every voxel on a tile face unites with its neighbours in other tiles in the global array.  Every access to the
//      array in this launch is a relaxed agent-scope atomic (the eight L2s are not coherent for plain accesses).  A stale parent would
//      only be an older ancestor and the hook compares against what the atomic returns; no workgroup waits for another.
//   3. cc_flatten_kernel: every voxel walks to its root and stores it.
// Parents only decrease, so every loop ends by construction; each has an iteration cap all the same, which sets the error word.
#include "common.h"

namespace rnerf {

constexpr int CC_TX = 8, CC_TY = 8, CC_TZ = 64, CC_LX = 3, CC_LY = 3, CC_LZ = 6;      // tile edges and their log2
constexpr int CC_TILE = CC_TX * CC_TY * CC_TZ, CC_THREADS = 256, CC_PER_THREAD = CC_TILE / CC_THREADS;
constexpr int CC_LDS_CAP = 2 * CC_TILE;            // a chain in a tile has at most CC_TILE links
constexpr int CC_FIND_CAP = 1 << 22, CC_UNION_CAP = 1 << 22;
constexpr int CC_STATS_SEGS = 32;                  // 64-voxel segments per wave of cc_stats_kernel

struct CCDims { int X, Y, Z, tx, ty, tz; };

// The 13 neighbours with a smaller linear index: k 0..8 = (-1, dy, dz), 9..11 = (0, -1, dz), 12 = (0, 0, -1).  Each adjacent pair is
// visited once, from its larger voxel.
__device__ __forceinline__ void cc_offset(int k, int& dx, int& dy, int& dz) {
  if (k < 9) { dx = -1; dy = k / 3 - 1; dz = k % 3 - 1; }
  else if (k < 12) { dx = 0; dy = -1; dz = k - 10; }
  else { dx = 0; dy = 0; dz = -1; }
}
template <int CONN>
__device__ __forceinline__ bool cc_adjacent(int dx, int dy, int dz) {
  const int nz = (dx != 0) + (dy != 0) + (dz != 0);
  return CONN == 26 || (CONN == 18 && nz <= 2) || nz == 1;
}

// ---- launch 1: LDS ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int lds_find(const int* par, int x, int& err) {
  for (int it = 0; it < CC_LDS_CAP; ++it) {
    const int p = lds_load(par + x);
    if (p == x) return x;
    x = p;
  }
  err = 1;
  return x;
}
__device__ __forceinline__ void lds_union(int* par, int a, int b, int& err) {
  for (int it = 0; it < CC_LDS_CAP && !err; ++it) {
    a = lds_find(par, a, err); b = lds_find(par, b, err);
    if (a == b || err) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == a) return;          // a was a root and now hangs under b
    a = old;                       // a had been hooked elsewhere in between: its old parent and b are still to be united
  }
  err = 1;
}

template <int CONN>
__global__ void __launch_bounds__(CC_THREADS) cc_tile_kernel(const uint8_t* __restrict__ solid, int phase, CCDims d, int* __restrict__ labels,
                                                             int* error) {
  __shared__ int par[CC_TILE];
  const int t = threadIdx.x;
  const unsigned b = blockIdx.x;
  const int x0 = (int)(b / ((unsigned)d.tz * d.ty)) << CC_LX, y0 = (int)((b / d.tz) % d.ty) << CC_LY, z0 = (int)(b % d.tz) << CC_LZ;
  unsigned mine = 0;               // bit j: voxel t + 256 j is of the labelled phase
  for (int j = 0; j < CC_PER_THREAD; ++j) {
    const int v = t + j * CC_THREADS;
    const int x = x0 + (v >> (CC_LY + CC_LZ)), y = y0 + ((v >> CC_LZ) & (CC_TY - 1)), z = z0 + (v & (CC_TZ - 1));
    bool on = false;
    if (x < d.X && y < d.Y && z < d.Z) on = (solid[((size_t)x * d.Y + y) * d.Z + z] != 0) == (phase != 0);
    par[v] = on ? v : -1;
    mine |= (unsigned)on << j;
  }
  __syncthreads();
  int err = 0;
  for (int j = 0; j < CC_PER_THREAD; ++j) {
    if (!((mine >> j) & 1u)) continue;
    const int v = t + j * CC_THREADS;
    const int lx = v >> (CC_LY + CC_LZ), ly = (v >> CC_LZ) & (CC_TY - 1), lz = v & (CC_TZ - 1);
#pragma unroll
    for (int k = 0; k < 13; ++k) {
      int dx, dy, dz;
      cc_offset(k, dx, dy, dz);
      if (!cc_adjacent<CONN>(dx, dy, dz)) continue;
      const int nx = lx + dx, ny = ly + dy, nz = lz + dz;
      if (nx < 0 || ny < 0 || ny >= CC_TY || nz < 0 || nz >= CC_TZ) continue;
      const int nv = (nx << (CC_LY + CC_LZ)) | (ny << CC_LZ) | nz;
      if (lds_load(par + nv) >= 0) lds_union(par, v, nv, err);      // -1 never changes
    }
  }
  __syncthreads();
  for (int j = 0; j < CC_PER_THREAD; ++j) {
    const int v = t + j * CC_THREADS;
    const int x = x0 + (v >> (CC_LY + CC_LZ)), y = y0 + ((v >> CC_LZ) & (CC_TY - 1)), z = z0 + (v & (CC_TZ - 1));
    if (!(x < d.X && y < d.Y && z < d.Z)) continue;
    int lab = -1;
    if ((mine >> j) & 1u) {
      const int r = lds_find(par, v, err);
      lab = (int)(((size_t)(x0 + (r >> (CC_LY + CC_LZ))) * d.Y + (y0 + ((r >> CC_LZ) & (CC_TY - 1)))) * d.Z + (z0 + (r & (CC_TZ - 1))));
    }
    labels[((size_t)x * d.Y + y) * d.Z + z] = lab;
  }
  if (err) atomicOr(error, 1);
}

// ---- launch 2: global, atomics only ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int agent_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int agent_find(int* par, int x, int& err) {
  for (int it = 0; it < CC_FIND_CAP; ++it) {
    const int p = agent_load(par + x);
    if (p == x) return x;
    x = p;
  }
  err = 1;
  return x;
}
__device__ __forceinline__ void agent_union(int* par, int a, int b, int& err) {
  for (int it = 0; it < CC_UNION_CAP && !err; ++it) {
    a = agent_find(par, a, err); b = agent_find(par, b, err);
    if (a == b || err) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;
  }
  err = 1;
}

// Uniform control flow down to the unions: a lane whose (own label, neighbour label) pair equals that of the lane before it (the voxel
// before it in z, in the same two tiles) leaves the union to that lane.  Across the face of two solid tiles that is one union per row
// instead of 64 on the same two roots.  Labels read later can only be smaller ancestors, so an equal pair names the same two trees.
template <int CONN>
__global__ void __launch_bounds__(CC_THREADS) cc_merge_kernel(CCDims d, unsigned n, int* labels, int* error) {
  const unsigned id = blockIdx.x * (unsigned)CC_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool active = id < n;
  int x = 0, y = 0, z = 0;
  if (active) {
    z = (int)(id % (unsigned)d.Z); y = (int)((id / (unsigned)d.Z) % (unsigned)d.Y); x = (int)(id / ((unsigned)d.Z * (unsigned)d.Y));
    const int lx = x & (CC_TX - 1), ly = y & (CC_TY - 1), lz = z & (CC_TZ - 1);
    if (lx > 0 && ly > 0 && ly < CC_TY - 1 && lz > 0 && lz < CC_TZ - 1) active = false;      // every smaller neighbour is in this voxel's own tile
  }
  if (!__any(active)) return;
  const int own = active ? agent_load(labels + id) : -1;
  active = own >= 0;
  int err = 0;
#pragma unroll
  for (int k = 0; k < 13; ++k) {
    int dx, dy, dz;
    cc_offset(k, dx, dy, dz);
    if (!cc_adjacent<CONN>(dx, dy, dz)) continue;          // compile-time
    const int nx = x + dx, ny = y + dy, nz = z + dz;
    bool v = active && nx >= 0 && ny >= 0 && ny < d.Y && nz >= 0 && nz < d.Z &&
             !((nx >> CC_LX) == (x >> CC_LX) && (ny >> CC_LY) == (y >> CC_LY) && (nz >> CC_LZ) == (z >> CC_LZ));      // same tile: united in LDS
    const int nid = v ? (int)(((size_t)nx * d.Y + ny) * d.Z + nz) : 0;
    const int nl = v ? agent_load(labels + nid) : -1;
    v = v && nl >= 0;
    const unsigned long long key = v ? (((unsigned long long)(unsigned)own << 32) | (unsigned)nl) : ~0ull;      // labels are < 2^31: no pair is ~0
    const unsigned long long before = __shfl_up(key, 1);
    if (v && !(lane > 0 && before == key)) agent_union(labels, (int)id, nid, err);
  }
  if (err) atomicOr(error, 1);
}

// ---- launch 3 -----------------------------------------------------------------------------------------------------------------------
// A voxel another thread has already flattened reads as its root, one not yet flattened as an ancestor: either leads to the same root,
// and a root's own entry never changes.
__global__ void __launch_bounds__(CC_THREADS) cc_flatten_kernel(unsigned n, int* labels, int* error) {
  const unsigned id = blockIdx.x * (unsigned)CC_THREADS + threadIdx.x;
  if (id >= n) return;
  int l = labels[id];
  if (l < 0) return;
  int it = 0;
  for (; it < CC_FIND_CAP; ++it) {
    const int p = labels[l];
    if (p == l) break;
    l = p;
  }
  if (it == CC_FIND_CAP) { atomicOr(error, 1); return; }
  labels[id] = l;
}

// ---- statistics ----------------------------------------------------------------------------------------------------------------------
// A wave walks CC_STATS_SEGS consecutive 64-voxel segments.  Per segment it groups its lanes by label with ballots; one label is
// carried in registers from segment to segment for as long as it keeps appearing (inside one component, or through a giant one that
// runs through the noise: one atomic per wave), the other groups add at once.
// Integer adds only: exact, whatever the order.
__global__ void __launch_bounds__(CC_THREADS) cc_stats_kernel(const int* __restrict__ labels, CCDims d, unsigned n, int* size, uint8_t* border,
                                                              unsigned long long* counts) {
  const int lane = threadIdx.x & 63;
  const unsigned long long wave = (unsigned long long)blockIdx.x * (CC_THREADS / 64) + (threadIdx.x >> 6);
  int held = -1, hcnt = 0;
  bool hborder = false;
  unsigned ncomp = 0, nvox = 0;
  for (int s = 0; s < CC_STATS_SEGS; ++s) {
    const unsigned long long base = (wave * CC_STATS_SEGS + s) * 64ull;
    if (base >= n) break;
    const unsigned long long i = base + lane;
    int l = -1;
    bool brd = false;
    if (i < n) {
      l = labels[i];
      const unsigned id = (unsigned)i;
      const int z = (int)(id % (unsigned)d.Z), y = (int)((id / (unsigned)d.Z) % (unsigned)d.Y), x = (int)(id / ((unsigned)d.Z * (unsigned)d.Y));
      brd = x == 0 || y == 0 || z == 0 || x == d.X - 1 || y == d.Y - 1 || z == d.Z - 1;
    }
    unsigned long long act = __ballot(l >= 0);
    nvox += (unsigned)__popcll(act);
    ncomp += (unsigned)__popcll(__ballot(l >= 0 && (unsigned long long)l == i));
    if (act && !(held >= 0 && __ballot(l == held))) {          // the carried label is not in this segment: carry the first one that is
      if (lane == 0 && held >= 0) { atomicAdd(size + held, hcnt); if (hborder) border[held] = 1; }
      held = __shfl(l, __ffsll((long long)act) - 1); hcnt = 0; hborder = false;
    }
    while (act) {
      const int lead = __shfl(l, __ffsll((long long)act) - 1);
      const unsigned long long m = __ballot(l == lead);
      const int c = __popcll(m);
      const bool bb = __ballot(l == lead && brd) != 0;
      if (lead == held) { hcnt += c; hborder |= bb; }
      else if (lane == 0) { atomicAdd(size + lead, c); if (bb) border[lead] = 1; }
      act &= ~m;
    }
  }
  if (lane == 0) {
    if (held >= 0) { atomicAdd(size + held, hcnt); if (hborder) border[held] = 1; }
    if (ncomp) atomicAdd(counts, (unsigned long long)ncomp);
    if (nvox) atomicAdd(counts + 1, (unsigned long long)nvox);
  }
}

// ---- apply ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(CC_THREADS) cc_apply_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ keep, T drop_value,
                                                              const int* __restrict__ fill_labels, const uint8_t* __restrict__ fill, T fill_value,
                                                              unsigned n, T* __restrict__ grid) {
  const unsigned id = blockIdx.x * (unsigned)CC_THREADS + threadIdx.x;
  if (id >= n) return;
  if (labels) {
    const int l = labels[id];
    if (l >= 0 && !keep[l]) grid[id] = drop_value;
  }
  if (fill_labels) {
    const int l = fill_labels[id];
    if (l >= 0 && fill[l]) grid[id] = fill_value;
  }
}

static bool cc_dims(const int32_t dims[3], CCDims* out, unsigned* n) {
  if (!dims) return false;
  long long total = 1;
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < 1) return false;
    total *= dims[a];
    if (total > 2147483647LL) return false;
  }
  CCDims d;
  d.X = dims[0]; d.Y = dims[1]; d.Z = dims[2];
  d.tx = (d.X + CC_TX - 1) / CC_TX; d.ty = (d.Y + CC_TY - 1) / CC_TY; d.tz = (d.Z + CC_TZ - 1) / CC_TZ;
  *out = d;
  *n = (unsigned)total;
  return true;
}
static unsigned cc_blocks(unsigned n) { return (unsigned)(((unsigned long long)n + CC_THREADS - 1) / CC_THREADS); }

constexpr size_t CC_WORKSPACE_BYTES = 64;      // word 0: the iteration-cap error word of the last rnerf_components_label

template <int CONN>
static void cc_launch_label(const uint8_t* solid, int phase, const CCDims& d, unsigned n, int* labels, int* error, hipStream_t s) {
  const unsigned tiles = (unsigned)d.tx * (unsigned)d.ty * (unsigned)d.tz;      // ceil(X/8) ceil(Y/8) ceil(Z/64) <= X Y Z < 2^31: fits a 1-D launch
  hipLaunchKernelGGL(cc_tile_kernel<CONN>, dim3(tiles), dim3(CC_THREADS), 0, s, solid, phase, d, labels, error);
  hipLaunchKernelGGL(cc_merge_kernel<CONN>, dim3(cc_blocks(n)), dim3(CC_THREADS), 0, s, d, n, labels, error);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(cc_blocks(n)), dim3(CC_THREADS), 0, s, n, labels, error);
}

}  // namespace rnerf

using namespace rnerf;

#define CC_DIMS_TEXT "need dims[0..2] >= 1 and dims[0] * dims[1] * dims[2] <= 2^31 - 1"

extern "C" size_t rnerf_components_workspace_bytes(const int32_t dims[3]) {
  CCDims d;
  unsigned n;
  if (!cc_dims(dims, &d, &n)) {
    set_error("rnerf_components_workspace_bytes: " CC_DIMS_TEXT);
    return 0;
  }
  return CC_WORKSPACE_BYTES;
}

extern "C" int rnerf_components_label(const uint8_t* solid, const int32_t dims[3], int32_t phase, int32_t connectivity, int32_t* labels,
                                      void* workspace, void* stream) {
  RNERF_CHECK_ARG(solid && dims && labels && workspace, "rnerf_components_label: null pointer");
  CCDims d;
  unsigned n;
  RNERF_CHECK_ARG(cc_dims(dims, &d, &n), "rnerf_components_label: " CC_DIMS_TEXT);
  RNERF_CHECK_ARG(phase == 0 || phase == 1, "rnerf_components_label: phase must be 0 (empty) or 1 (solid)");
  RNERF_CHECK_ARG(connectivity == 6 || connectivity == 18 || connectivity == 26, "rnerf_components_label: connectivity must be 6, 18 or 26, got %d",
                  connectivity);
  RNERF_CHECK_ARG(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)labels & 3) == 0, "rnerf_components_label: labels and workspace must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  RNERF_CHECK_HIP(hipMemsetAsync(workspace, 0, CC_WORKSPACE_BYTES, s));
  int* error = (int*)workspace;
  if (connectivity == 6) cc_launch_label<6>(solid, phase, d, n, labels, error, s);
  else if (connectivity == 18) cc_launch_label<18>(solid, phase, d, n, labels, error, s);
  else cc_launch_label<26>(solid, phase, d, n, labels, error, s);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_components_stats(const int32_t* labels, const int32_t dims[3], int32_t* size, uint8_t* border, int64_t* counts, void* stream) {
  RNERF_CHECK_ARG(labels && dims && size && border && counts, "rnerf_components_stats: null pointer");
  CCDims d;
  unsigned n;
  RNERF_CHECK_ARG(cc_dims(dims, &d, &n), "rnerf_components_stats: " CC_DIMS_TEXT);
  RNERF_CHECK_ARG(((uintptr_t)size & 3) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)counts & 7) == 0,
                  "rnerf_components_stats: labels and size must be 4-byte, counts 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  RNERF_CHECK_HIP(hipMemsetAsync(size, 0, (size_t)n * sizeof(int32_t), s));
  RNERF_CHECK_HIP(hipMemsetAsync(border, 0, (size_t)n, s));
  RNERF_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s));
  const unsigned long long per_block = 64ull * CC_STATS_SEGS * (CC_THREADS / 64);
  hipLaunchKernelGGL(cc_stats_kernel, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(CC_THREADS), 0, s, labels, d, n, size, border,
                     (unsigned long long*)counts);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_components_apply(const int32_t* labels, const uint8_t* keep, double drop_value, const int32_t* fill_labels, const uint8_t* fill,
                                      double fill_value, void* grid, int32_t dtype, const int32_t dims[3], void* stream) {
  RNERF_CHECK_ARG(grid && dims, "rnerf_components_apply: null pointer");
  RNERF_CHECK_ARG((labels != nullptr) == (keep != nullptr) && (fill_labels != nullptr) == (fill != nullptr) && (labels || fill_labels),
                  "rnerf_components_apply: labels and keep, fill_labels and fill go in pairs, and one pair is needed");
  CCDims d;
  unsigned n;
  RNERF_CHECK_ARG(cc_dims(dims, &d, &n), "rnerf_components_apply: " CC_DIMS_TEXT);
  RNERF_CHECK_ARG(dtype == RNERF_COMPONENTS_U8 || dtype == RNERF_COMPONENTS_I32 || dtype == RNERF_COMPONENTS_F32,
                  "rnerf_components_apply: dtype must be RNERF_COMPONENTS_U8, _I32 or _F32, got %d", dtype);
  RNERF_CHECK_ARG(dtype == RNERF_COMPONENTS_U8 || ((uintptr_t)grid & 3) == 0, "rnerf_components_apply: grid must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const dim3 blocks(cc_blocks(n)), threads(CC_THREADS);
  if (dtype == RNERF_COMPONENTS_U8)
    hipLaunchKernelGGL(cc_apply_kernel<uint8_t>, blocks, threads, 0, s, labels, keep, (uint8_t)drop_value, fill_labels, fill, (uint8_t)fill_value, n, (uint8_t*)grid);
  else if (dtype == RNERF_COMPONENTS_I32)
    hipLaunchKernelGGL(cc_apply_kernel<int32_t>, blocks, threads, 0, s, labels, keep, (int32_t)drop_value, fill_labels, fill, (int32_t)fill_value, n, (int32_t*)grid);
  else
    hipLaunchKernelGGL(cc_apply_kernel<float>, blocks, threads, 0, s, labels, keep, (float)drop_value, fill_labels, fill, (float)fill_value, n, (float*)grid);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}
