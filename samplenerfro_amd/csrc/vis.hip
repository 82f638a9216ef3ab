// Depth visualisations of rnerf/vis.py on the device: rnerf_vis_depth (visualize_depth, :45-111) and rnerf_vis_normals
// (depth_to_normals + visualize_normals, :34-42, 114-132).  float32 per pixel in the order of the reference's formulas; every reduction
// is a fixed-order sum / minimum of per-block partials, the sort is an LSD radix sort with integer histograms: no float atomics, the same
// bytes on every run.
#include <math.h>

#include "common.h"
#include "eval_host.h"
#include "turbo_table.h"

namespace rnerf {
namespace {

constexpr int VIS_THREADS = 256;
constexpr int VIS_WAVES = VIS_THREADS / 64;
constexpr int VIS_MAX_PARTIALS = 256;          // reduction grids: at most this many blocks, so a consumer block folds them with one load per thread
constexpr int VIS_SORT_MIN_TILE = 4096;        // elements per sort block (a multiple of VIS_THREADS); grows so that there are at most 1024 blocks
constexpr int VIS_SORT_MAX_BLOCKS = 1024;
constexpr float VIS_EPS = 1.1920928955078125e-07f;      // jnp.finfo(jnp.float32).eps = 2^-23
constexpr float VIS_PI = 3.14159265358979323846f;

__constant__ float turbo_table[256][3] = RNERF_TURBO_TABLE;

struct VisRange { float mn, mx; unsigned has_nan, count; };      // per block: min / max over the non-NaN depths, a NaN seen, non-NaN seen (saturating)
struct VisMoments { double a, b, c, n; };

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// sum of one VisMoments per thread over the block, in a fixed order; valid in every thread afterwards.  s: [VIS_WAVES + 1]
__device__ __forceinline__ VisMoments block_sum(VisMoments v, VisMoments* s) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  v.a = wave_sum_d(v.a); v.b = wave_sum_d(v.b); v.c = wave_sum_d(v.c); v.n = wave_sum_d(v.n);
  __syncthreads();                                     // s may still be read from an earlier call
  if (lane == 0) s[wave] = v;
  __syncthreads();
  if (tid == 0) {
    VisMoments t = s[0];
    for (int w = 1; w < VIS_WAVES; ++w) { t.a += s[w].a; t.b += s[w].b; t.c += s[w].c; t.n += s[w].n; }
    s[VIS_WAVES] = t;
  }
  __syncthreads();
  return s[VIS_WAVES];
}

__device__ __forceinline__ VisRange range_merge(VisRange p, VisRange q) {
  VisRange r;
  r.mn = q.mn < p.mn ? q.mn : p.mn; r.mx = q.mx > p.mx ? q.mx : p.mx;
  r.has_nan = p.has_nan | q.has_nan; r.count = p.count | q.count;
  return r;
}

__device__ __forceinline__ VisRange block_range(VisRange v, VisRange* s) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    VisRange q;
    q.mn = __shfl_down(v.mn, o, 64); q.mx = __shfl_down(v.mx, o, 64);
    q.has_nan = __shfl_down(v.has_nan, o, 64); q.count = __shfl_down(v.count, o, 64);
    v = range_merge(v, q);
  }
  __syncthreads();
  if (lane == 0) s[wave] = v;
  __syncthreads();
  if (tid == 0) {
    VisRange t = s[0];
    for (int w = 1; w < VIS_WAVES; ++w) t = range_merge(t, s[w]);
    s[VIS_WAVES] = t;
  }
  __syncthreads();
  return s[VIS_WAVES];
}

__device__ __forceinline__ VisRange range_identity() { return VisRange{INFINITY, -INFINITY, 0u, 0u}; }

// ---- the automatic range with ignore_frac == 0: one reduction ------------------------------------------------------------------
__global__ __launch_bounds__(VIS_THREADS) void vis_minmax_kernel(const float* __restrict__ depth, long long N, VisRange* __restrict__ partials) {
  __shared__ VisRange s[VIS_WAVES + 1];
  VisRange v = range_identity();
  for (long long i = (long long)blockIdx.x * VIS_THREADS + threadIdx.x; i < N; i += (long long)gridDim.x * VIS_THREADS) {
    const float d = depth[i];
    if (d != d) { v.has_nan = 1u; continue; }
    v.mn = d < v.mn ? d : v.mn; v.mx = d > v.mx ? d : v.mx; v.count = 1u;
  }
  v = block_range(v, s);
  if (threadIdx.x == 0) partials[blockIdx.x] = v;
}

// ---- the automatic range with ignore_frac > 0: stable LSD radix sort of (key, pixel index), then a fixed-order fp64 scan of acc' -------
// Orderable key: ascending like the float, -0 with +0 (jnp.argsort compares them equal; the index decides), every NaN last.
__device__ __forceinline__ unsigned vis_key(float d) {
  if (d != d) return 0xFFFFFFFFu;
  if (d == 0.f) return 0x80000000u;
  const unsigned u = __float_as_uint(d);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(VIS_THREADS) void vis_keys_kernel(const float* __restrict__ depth, long long N, unsigned* __restrict__ keys,
                                                               unsigned* __restrict__ idx) {
  const long long i = (long long)blockIdx.x * VIS_THREADS + threadIdx.x;
  if (i >= N) return;
  keys[i] = vis_key(depth[i]);
  idx[i] = (unsigned)i;
}

__global__ __launch_bounds__(VIS_THREADS) void vis_hist_kernel(const unsigned* __restrict__ keys, long long N, long long tile, int shift,
                                                               unsigned* __restrict__ hist) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const long long lo = (long long)blockIdx.x * tile, hi = lo + tile < N ? lo + tile : N;
  for (long long i = lo + threadIdx.x; i < hi; i += VIS_THREADS) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);      // integer, in LDS: the counts are exact
  __syncthreads();
  hist[(long long)blockIdx.x * 256 + threadIdx.x] = h[threadIdx.x];
}

// Block b's elements of digit d go to [sum of every block's count of the lower digits + the earlier blocks' count of d, ...), in their
// order in the block: the rank inside a round of VIS_THREADS elements is the number of lower lanes (ballots) and lower waves with that digit.
__global__ __launch_bounds__(VIS_THREADS) void vis_scatter_kernel(const unsigned* __restrict__ keys_in, const unsigned* __restrict__ idx_in,
                                                                  unsigned* __restrict__ keys_out, unsigned* __restrict__ idx_out, long long N,
                                                                  long long tile, int shift, const unsigned* __restrict__ hist) {
  __shared__ unsigned s_tot[256], s_base[256], s_cnt[VIS_WAVES][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, nb = gridDim.x;
  unsigned tot = 0u, mine = 0u;
  for (int q = 0; q < nb; ++q) {
    const unsigned v = hist[(long long)q * 256 + tid];
    if (q < b) mine += v;
    tot += v;
  }
  s_tot[tid] = tot;
#pragma unroll
  for (int w = 0; w < VIS_WAVES; ++w) s_cnt[w][tid] = 0u;
  __syncthreads();
  unsigned below = 0u;
  for (int d = 0; d < tid; ++d) below += s_tot[d];
  s_base[tid] = below + mine;
  __syncthreads();
  const long long lo = (long long)b * tile, hi = lo + tile < N ? lo + tile : N;
  for (long long r = lo; r < hi; r += VIS_THREADS) {
    const long long i = r + tid;
    const bool valid = i < hi;
    const unsigned key = valid ? keys_in[i] : 0u;
    const unsigned d = (key >> shift) & 255u;
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (d >> bit) & 1u;
      const unsigned long long m = __ballot(valid && on);
      same &= on ? m : ~m;
    }
    const unsigned rank = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
    if (valid && rank == 0u) s_cnt[wave][d] = (unsigned)__popcll(same);
    __syncthreads();
    if (valid) {
      unsigned off = s_base[d] + rank;
      for (int w = 0; w < wave; ++w) off += s_cnt[w][d];
      if ((long long)off < N) {          // always true for a histogram of these keys; keeps a store inside the buffer whatever it holds
        keys_out[off] = key;
        idx_out[off] = idx_in[i];
      }
    }
    __syncthreads();
    unsigned add = 0u;
#pragma unroll
    for (int w = 0; w < VIS_WAVES; ++w) { add += s_cnt[w][tid]; s_cnt[w][tid] = 0u; }
    s_base[tid] += add;
    __syncthreads();
  }
}

__device__ __forceinline__ double vis_weight(const float* __restrict__ depth, const float* __restrict__ acc, long long N, unsigned j) {
  if ((long long)j >= N) return 0.0;                   // never for the sorted permutation; keeps a load inside the plane whatever idx holds
  const float d = depth[j];
  return d != d ? 0.0 : (acc ? (double)acc[j] : 1.0);
}

// Sorted positions [lo, hi) of a block, a contiguous chunk per thread: the thread's sum, then its exclusive prefix inside the block
// (thread 0 adds the VIS_THREADS sums in order).  s: [VIS_THREADS + 1], s[VIS_THREADS] = the block's sum.
__device__ __forceinline__ double vis_chunk_prefix(const unsigned* __restrict__ idx, const float* __restrict__ depth, const float* __restrict__ acc,
                                                   long long N, long long c0, long long c1, double* s) {
  double sum = 0.0;
  for (long long k = c0; k < c1; ++k) sum += vis_weight(depth, acc, N, idx[k]);
  s[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double run = 0.0;
    for (int t = 0; t < VIS_THREADS; ++t) { const double v = s[t]; s[t] = run; run += v; }
    s[VIS_THREADS] = run;
  }
  __syncthreads();
  return s[threadIdx.x];
}

__global__ __launch_bounds__(VIS_THREADS) void vis_cum_partial_kernel(const unsigned* __restrict__ idx, const float* __restrict__ depth,
                                                                      const float* __restrict__ acc, long long N, long long tile,
                                                                      double* __restrict__ partials) {
  __shared__ double s[VIS_THREADS + 1];
  const long long lo = (long long)blockIdx.x * tile, hi = lo + tile < N ? lo + tile : N, per = tile / VIS_THREADS;
  long long c0 = lo + threadIdx.x * per, c1 = c0 + per;
  c0 = c0 < hi ? c0 : hi; c1 = c1 < hi ? c1 : hi;
  vis_chunk_prefix(idx, depth, acc, N, c0, c1, s);
  if (threadIdx.x == 0) partials[blockIdx.x] = s[VIS_THREADS];
}

// cum = the inclusive running sum of acc' in sorted order: (sum of the earlier blocks' sums + the thread's prefix) + the chunk's elements
// one by one; total = the sum of every block's sum.  Per block: the first and one past the last kept position (0 = none).
__global__ __launch_bounds__(VIS_THREADS) void vis_select_kernel(const unsigned* __restrict__ idx, const float* __restrict__ depth,
                                                                 const float* __restrict__ acc, long long N, long long tile,
                                                                 const double* __restrict__ partials, double ignore_frac,
                                                                 unsigned* __restrict__ sel) {
  __shared__ double s[VIS_THREADS + 1];
  __shared__ double s_pre[2];
  __shared__ unsigned s_first, s_last;
  if (threadIdx.x == 0) {
    double run = 0.0, pre = 0.0;
    for (unsigned q = 0; q < gridDim.x; ++q) {
      if (q == blockIdx.x) pre = run;
      run += partials[q];
    }
    s_pre[0] = pre; s_pre[1] = run;
    s_first = 0xFFFFFFFFu; s_last = 0u;
  }
  const long long lo = (long long)blockIdx.x * tile, hi = lo + tile < N ? lo + tile : N, per = tile / VIS_THREADS;
  long long c0 = lo + threadIdx.x * per, c1 = c0 + per;
  c0 = c0 < hi ? c0 : hi; c1 = c1 < hi ? c1 : hi;
  const double excl = vis_chunk_prefix(idx, depth, acc, N, c0, c1, s);      // its barriers also publish s_pre, s_first, s_last
  const double total = s_pre[1], t_lo = total * ignore_frac, t_hi = total * (1.0 - ignore_frac);
  double cum = s_pre[0] + excl;
  unsigned first = 0xFFFFFFFFu, last = 0u;
  for (long long k = c0; k < c1; ++k) {
    cum += vis_weight(depth, acc, N, idx[k]);
    if (cum >= t_lo && cum <= t_hi) {
      if (first == 0xFFFFFFFFu) first = (unsigned)k;
      last = (unsigned)k + 1u;
    }
  }
  if (last != 0u) { atomicMin(&s_first, first); atomicMax(&s_last, last); }
  __syncthreads();
  if (threadIdx.x == 0) { sel[2 * blockIdx.x] = s_first; sel[2 * blockIdx.x + 1] = s_last; }
}

// One block: the first and last kept depth as the single VisRange the map kernel folds (nothing kept: both bounds NaN).
__global__ __launch_bounds__(VIS_THREADS) void vis_select_final_kernel(const unsigned* __restrict__ sel, int nb, const unsigned* __restrict__ idx,
                                                                       const float* __restrict__ depth, long long N, VisRange* __restrict__ out) {
  __shared__ unsigned s_first, s_last;
  if (threadIdx.x == 0) { s_first = 0xFFFFFFFFu; s_last = 0u; }
  __syncthreads();
  unsigned first = 0xFFFFFFFFu, last = 0u;
  for (int q = threadIdx.x; q < nb; q += VIS_THREADS) {
    if (sel[2 * q + 1] == 0u) continue;
    first = sel[2 * q] < first ? sel[2 * q] : first;
    last = sel[2 * q + 1] > last ? sel[2 * q + 1] : last;
  }
  if (last != 0u) { atomicMin(&s_first, first); atomicMax(&s_last, last); }
  __syncthreads();
  if (threadIdx.x == 0) {
    VisRange r = range_identity();
    r.has_nan = 1u;
    const unsigned jn = s_last != 0u ? idx[s_first] : 0u, jf = s_last != 0u ? idx[s_last - 1u] : 0u;
    if (s_last != 0u && (long long)jn < N && (long long)jf < N) {
      const float dn = depth[jn], df = depth[jf];
      if (dn == dn) { r.mn = dn; r.count = 1u; }
      r.has_nan = df != df ? 1u : 0u;
      r.mx = df;
    }
    out[0] = r;
  }
}

// ---- the per-pixel map ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float vis_curve(float x, int curve) {
  switch (curve) {
    case RNERF_VIS_CURVE_IDENTITY: return x;
    case RNERF_VIS_CURVE_RECIPROCAL: return 1.0f / (x + VIS_EPS);
    case RNERF_VIS_CURVE_LOG: return logf(x + VIS_EPS);
    default: return -logf(x + VIS_EPS);
  }
}

__device__ __forceinline__ float vis_sin2(float x) { const float s = sinf(VIS_PI * x); return s * s; }

__global__ __launch_bounds__(VIS_THREADS) void vis_depth_map_kernel(const float* __restrict__ depth, const float* __restrict__ acc, long long N,
                                                                    float near_given, float far_given, int have_near, int have_far,
                                                                    const VisRange* __restrict__ partials, int num_partials, int curve,
                                                                    float modulus, float* __restrict__ rgb, float* __restrict__ value,
                                                                    float* __restrict__ range) {
  __shared__ VisRange s[VIS_WAVES + 1];
  float near = near_given, far = far_given;
  if (!(have_near && have_far)) {
    const VisRange r = block_range(threadIdx.x < num_partials ? partials[threadIdx.x] : range_identity(), s);
    // depth_keep[0] - eps, depth_keep[-1] + eps (vis.py:89-91): NaN sorts last, so it is the far bound wherever there is one
    if (!have_near) near = r.count ? r.mn - VIS_EPS : NAN;
    if (!have_far) far = r.has_nan ? NAN : r.mx + VIS_EPS;
  }
  const long long i = (long long)blockIdx.x * VIS_THREADS + threadIdx.x;
  if (range && i == 0) { range[0] = near; range[1] = far; }
  if (i >= N || !(rgb || value)) return;
  const float d0 = depth[i];
  const float a = d0 != d0 ? 0.f : (acc ? acc[i] : 1.f);
  const float d = vis_curve(d0, curve);
  float v, cr, cg, cb;
  if (modulus > 0.f) {
    float m = fmodf(d, modulus);                       // jnp.mod: the remainder takes the divisor's sign
    if (m != 0.f && m < 0.f) m = m + modulus;
    v = m / modulus;
    cr = vis_sin2(0.5f - v); cg = vis_sin2((float)(5.0 / 6.0) - v); cb = vis_sin2((float)(7.0 / 6.0) - v);
  } else {
    const float n = vis_curve(near, curve), f = vis_curve(far, curve);
    const float lo = (n != n || f != f) ? NAN : (n < f ? n : f);
    v = (d - lo) / fabsf(f - n);
    v = v != v ? 0.f : (v < 0.f ? 0.f : (v > 1.f ? 1.f : v));      // nan_to_num(clip(., 0, 1))
    int t = (int)(v * 256.f);
    t = t > 255 ? 255 : t;
    cr = turbo_table[t][0]; cg = turbo_table[t][1]; cb = turbo_table[t][2];
  }
  if (value) value[i] = v;
  if (rgb) {
    const float w = 1.f - a;
    rgb[3 * i] = cr * a + w; rgb[3 * i + 1] = cg * a + w; rgb[3 * i + 2] = cb * a + w;
  }
}

// ---- normals: the automatic scaling (two passes of fp64 sums over the non-NaN pixels), then the 3 x 3 convolutions -------------------
__global__ __launch_bounds__(VIS_THREADS) void vis_moments1_kernel(const float* __restrict__ depth, long long N, int W, VisMoments* __restrict__ partials) {
  __shared__ VisMoments s[VIS_WAVES + 1];
  VisMoments v = {0.0, 0.0, 0.0, 0.0};
  for (long long i = (long long)blockIdx.x * VIS_THREADS + threadIdx.x; i < N; i += (long long)gridDim.x * VIS_THREADS) {
    const float d = depth[i];
    if (d != d) continue;
    const long long r = i / W;
    v.a += (double)(i - r * W); v.b += (double)r; v.c += (double)d; v.n += 1.0;
  }
  v = block_sum(v, s);
  if (threadIdx.x == 0) partials[blockIdx.x] = v;
}

__global__ __launch_bounds__(VIS_THREADS) void vis_moments2_kernel(const float* __restrict__ depth, long long N, int W,
                                                                   const VisMoments* __restrict__ first, VisMoments* __restrict__ partials) {
  __shared__ VisMoments s[VIS_WAVES + 1];
  const VisMoments zero = {0.0, 0.0, 0.0, 0.0};
  const VisMoments m = block_sum(threadIdx.x < gridDim.x ? first[threadIdx.x] : zero, s);      // this grid is the first pass's
  const double mx = m.a / m.n, my = m.b / m.n, mz = m.c / m.n;
  VisMoments v = zero;
  for (long long i = (long long)blockIdx.x * VIS_THREADS + threadIdx.x; i < N; i += (long long)gridDim.x * VIS_THREADS) {
    const float d = depth[i];
    if (d != d) continue;
    const long long r = i / W;
    const double ex = (double)(i - r * W) - mx, ey = (double)r - my, ez = (double)d - mz;
    v.a += ex * ex; v.b += ey * ey; v.c += ez * ez; v.n += 1.0;
  }
  v = block_sum(v, s);
  if (threadIdx.x == 0) partials[blockIdx.x] = v;
}

__device__ __forceinline__ float vis_normal_colour(float n) {
  const float h = (n + 1.0f) / 2.0f;                   // isnan(n) + nan_to_num((n + 1) / 2): a NaN component is 1
  return n != n ? 1.0f : (h == INFINITY ? 3.4028234663852886e38f : (h == -INFINITY ? -3.4028234663852886e38f : h));
}

__global__ __launch_bounds__(VIS_THREADS) void vis_normals_map_kernel(const float* __restrict__ depth, const float* __restrict__ acc, int H, int W,
                                                                      float scaling_given, const VisMoments* __restrict__ second,
                                                                      int num_partials, float* __restrict__ rgb, float* __restrict__ normals) {
  __shared__ VisMoments s[VIS_WAVES + 1];
  float scaling = scaling_given;
  if (second) {
    const VisMoments zero = {0.0, 0.0, 0.0, 0.0};
    const VisMoments m = block_sum(threadIdx.x < num_partials ? second[threadIdx.x] : zero, s);
    scaling = (float)sqrt((((m.a / m.n) + (m.b / m.n)) / 2.0) / (m.c / m.n));      // population variances; rounded to float32 once
  }
  const long long N = (long long)H * W, i = (long long)blockIdx.x * VIS_THREADS + threadIdx.x;
  if (i >= N) return;
  const int r = (int)(i / W), c = (int)(i - (long long)r * W);
  // convolve2d(z, k, mode='same'): out[r][c] = sum over (p, q) of k[p][q] z[r + 1 - p][c + 1 - q], zero outside, in kernel order, all
  // nine products formed.  ky = edge (x) blur = [-1, 0, 1]^T / 2 (x) [1, 2, 1] / 4 (vis.py:38), kx its transpose (:39).
  const float edge[3] = {-0.5f, 0.f, 0.5f}, blur[3] = {0.25f, 0.5f, 0.25f};
  float dy = 0.f, dx = 0.f;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int rr = r + 1 - p, cc = c + 1 - q;
      const float z = (rr >= 0 && rr < H && cc >= 0 && cc < W) ? scaling * depth[(long long)rr * W + cc] : 0.f;
      dy = dy + (edge[p] * blur[q]) * z;
      dx = dx + (blur[p] * edge[q]) * z;
    }
  }
  const float inv = 1.0f / sqrtf((1.0f + dx * dx) + dy * dy);
  const float n0 = dx * inv, n1 = dy * inv;
  if (normals) { normals[3 * i] = n0; normals[3 * i + 1] = n1; normals[3 * i + 2] = inv; }
  if (rgb) {
    float c0 = vis_normal_colour(n0), c1 = vis_normal_colour(n1), c2 = vis_normal_colour(inv);
    if (acc) {                                         // the raw acc: not zeroed at a NaN depth here (vis.py:129-130)
      const float a = acc[i], w = 1.f - a;
      c0 = c0 * a + w; c1 = c1 * a + w; c2 = c2 * a + w;
    }
    rgb[3 * i] = c0; rgb[3 * i + 1] = c1; rgb[3 * i + 2] = c2;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
inline int reduce_blocks(long long N) { const long long b = (N + VIS_THREADS - 1) / VIS_THREADS; return (int)(b < VIS_MAX_PARTIALS ? b : VIS_MAX_PARTIALS); }

struct SortPlan { long long tile; int nb; };
inline SortPlan sort_plan(long long N) {
  SortPlan p;
  p.tile = VIS_SORT_MIN_TILE;
  const long long need = (N + VIS_SORT_MAX_BLOCKS - 1) / VIS_SORT_MAX_BLOCKS;
  if (need > p.tile) p.tile = (need + VIS_THREADS - 1) / VIS_THREADS * VIS_THREADS;
  p.nb = (int)((N + p.tile - 1) / p.tile);
  return p;
}

// workspace of rnerf_vis_depth: [VisRange x VIS_MAX_PARTIALS] and, for the sort, [keys x 2][idx x 2][hist][cum partials][sel]
struct DepthLayout { size_t ranges, keys, idx, hist, cum, sel, total; };
inline DepthLayout depth_layout(long long N, bool sort) {
  DepthLayout l = {};
  size_t at = 0;
  l.ranges = at; at += up16(sizeof(VisRange) * VIS_MAX_PARTIALS);
  if (sort) {
    const SortPlan p = sort_plan(N);
    l.keys = at; at += 2 * up16(sizeof(unsigned) * (size_t)N);
    l.idx = at; at += 2 * up16(sizeof(unsigned) * (size_t)N);
    l.hist = at; at += up16(sizeof(unsigned) * 256 * (size_t)p.nb);
    l.cum = at; at += up16(sizeof(double) * (size_t)p.nb);
    l.sel = at; at += up16(sizeof(unsigned) * 2 * (size_t)p.nb);
  }
  l.total = at;
  return l;
}

int vis_check_size(const char* who, int32_t H, int32_t W) {
  RNERF_CHECK_ARG(H >= 1 && W >= 1, "%s: need H >= 1 and W >= 1", who);
  RNERF_CHECK_ARG((long long)H * W < (1LL << 31), "%s: H * W must be below 2^31", who);
  return RNERF_OK;
}

int vis_check_frac(double ignore_frac) {
  RNERF_CHECK_ARG(isfinite(ignore_frac) && ignore_frac >= 0.0 && ignore_frac < 0.5, "rnerf_vis_depth: ignore_frac must be in [0, 0.5)");
  return RNERF_OK;
}

}  // namespace
}  // namespace rnerf

using namespace rnerf;

extern "C" size_t rnerf_vis_depth_workspace_bytes(int32_t H, int32_t W, double ignore_frac) {
  if (vis_check_size("rnerf_vis_depth", H, W) != RNERF_OK || vis_check_frac(ignore_frac) != RNERF_OK) return 0;
  return depth_layout((long long)H * W, ignore_frac > 0.0).total;
}

extern "C" int rnerf_vis_depth(const float* depth, const float* acc, int32_t H, int32_t W, double near, double far, double ignore_frac, int32_t curve,
                               double modulus, float* rgb, float* value, float* range, void* workspace, void* stream) {
  int rc = vis_check_size("rnerf_vis_depth", H, W);
  if (rc != RNERF_OK) return rc;
  if ((rc = vis_check_frac(ignore_frac)) != RNERF_OK) return rc;
  RNERF_CHECK_ARG(depth && (rgb || value || range), "rnerf_vis_depth: null pointer (depth, and rgb, value or range)");
  RNERF_CHECK_ARG(isfinite(modulus) && modulus >= 0.0, "rnerf_vis_depth: modulus must be finite and >= 0");
  RNERF_CHECK_ARG(curve >= RNERF_VIS_CURVE_NEG_LOG && curve <= RNERF_VIS_CURVE_LOG, "rnerf_vis_depth: unknown curve %d", curve);
  const bool have_near = !isnan(near), have_far = !isnan(far), need_auto = !(have_near && have_far);
  RNERF_CHECK_ARG(!need_auto || workspace, "rnerf_vis_depth: an automatic near or far needs the workspace (rnerf_vis_depth_workspace_bytes)");
  RNERF_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "rnerf_vis_depth: the workspace must be 16-byte aligned");
  const long long N = (long long)H * W;
  const size_t plane = (size_t)N * sizeof(float);
  const void* ins[2] = {depth, acc};
  for (const void* in : ins)
    RNERF_CHECK_ARG(!overlaps(in, plane, rgb, 3 * plane) && !overlaps(in, plane, value, plane) && !overlaps(in, plane, range, 2 * sizeof(float)),
                    "rnerf_vis_depth: an output overlaps depth or acc");
  RNERF_CHECK_ARG(!overlaps(rgb, 3 * plane, value, plane) && !overlaps(rgb, 3 * plane, range, 8) && !overlaps(value, plane, range, 8),
                  "rnerf_vis_depth: the outputs overlap each other");
  hipStream_t st = (hipStream_t)stream;
  const bool sort = need_auto && ignore_frac > 0.0;
  const DepthLayout l = depth_layout(N, sort);
  char* ws = (char*)workspace;
  VisRange* ranges = need_auto ? (VisRange*)(ws + l.ranges) : nullptr;
  int num_partials = 0;
  const unsigned pixel_blocks = (unsigned)((N + VIS_THREADS - 1) / VIS_THREADS);
  if (need_auto && !sort) {
    num_partials = reduce_blocks(N);
    hipLaunchKernelGGL(vis_minmax_kernel, dim3(num_partials), dim3(VIS_THREADS), 0, st, depth, N, ranges);
    RNERF_CHECK_LAUNCH();
  } else if (sort) {
    const SortPlan p = sort_plan(N);
    const size_t stride = up16(sizeof(unsigned) * (size_t)N);
    unsigned* keys[2] = {(unsigned*)(ws + l.keys), (unsigned*)(ws + l.keys + stride)};
    unsigned* idx[2] = {(unsigned*)(ws + l.idx), (unsigned*)(ws + l.idx + stride)};
    unsigned* hist = (unsigned*)(ws + l.hist);
    double* cum = (double*)(ws + l.cum);
    unsigned* sel = (unsigned*)(ws + l.sel);
    hipLaunchKernelGGL(vis_keys_kernel, dim3(pixel_blocks), dim3(VIS_THREADS), 0, st, depth, N, keys[0], idx[0]);
    RNERF_CHECK_LAUNCH();
    for (int pass = 0; pass < 4; ++pass) {
      const int from = pass & 1, to = from ^ 1;
      hipLaunchKernelGGL(vis_hist_kernel, dim3(p.nb), dim3(VIS_THREADS), 0, st, keys[from], N, p.tile, 8 * pass, hist);
      RNERF_CHECK_LAUNCH();
      hipLaunchKernelGGL(vis_scatter_kernel, dim3(p.nb), dim3(VIS_THREADS), 0, st, keys[from], idx[from], keys[to], idx[to], N, p.tile, 8 * pass, hist);
      RNERF_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(vis_cum_partial_kernel, dim3(p.nb), dim3(VIS_THREADS), 0, st, idx[0], depth, acc, N, p.tile, cum);
    RNERF_CHECK_LAUNCH();
    hipLaunchKernelGGL(vis_select_kernel, dim3(p.nb), dim3(VIS_THREADS), 0, st, idx[0], depth, acc, N, p.tile, cum, ignore_frac, sel);
    RNERF_CHECK_LAUNCH();
    hipLaunchKernelGGL(vis_select_final_kernel, dim3(1), dim3(VIS_THREADS), 0, st, sel, p.nb, idx[0], depth, N, ranges);
    RNERF_CHECK_LAUNCH();
    num_partials = 1;
  }
  const unsigned grid = (rgb || value) ? pixel_blocks : 1u;
  hipLaunchKernelGGL(vis_depth_map_kernel, dim3(grid), dim3(VIS_THREADS), 0, st, depth, acc, N, (float)near, (float)far, (int)have_near, (int)have_far,
                     ranges, num_partials, (int)curve, (float)modulus, rgb, value, range);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" size_t rnerf_vis_normals_workspace_bytes(int32_t H, int32_t W) {
  if (vis_check_size("rnerf_vis_normals", H, W) != RNERF_OK) return 0;
  return 2 * up16(sizeof(VisMoments) * VIS_MAX_PARTIALS);
}

extern "C" int rnerf_vis_normals(const float* depth, const float* acc, int32_t H, int32_t W, double scaling, float* rgb, float* normals,
                                 void* workspace, void* stream) {
  const int rc = vis_check_size("rnerf_vis_normals", H, W);
  if (rc != RNERF_OK) return rc;
  RNERF_CHECK_ARG(depth && (rgb || normals), "rnerf_vis_normals: null pointer (depth, and rgb or normals)");
  const bool need_auto = isnan(scaling);
  RNERF_CHECK_ARG(!need_auto || workspace, "rnerf_vis_normals: the automatic scaling needs the workspace (rnerf_vis_normals_workspace_bytes)");
  RNERF_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "rnerf_vis_normals: the workspace must be 16-byte aligned");
  const long long N = (long long)H * W;
  const size_t plane = (size_t)N * sizeof(float);
  RNERF_CHECK_ARG(!overlaps(depth, plane, rgb, 3 * plane) && !overlaps(acc, plane, rgb, 3 * plane) && !overlaps(depth, plane, normals, 3 * plane) &&
                      !overlaps(acc, plane, normals, 3 * plane) && !overlaps(rgb, 3 * plane, normals, 3 * plane),
                  "rnerf_vis_normals: an output overlaps depth, acc or the other output");
  hipStream_t st = (hipStream_t)stream;
  VisMoments* second = nullptr;
  int num_partials = 0;
  if (need_auto) {
    VisMoments* first = (VisMoments*)workspace;
    second = (VisMoments*)((char*)workspace + up16(sizeof(VisMoments) * VIS_MAX_PARTIALS));
    num_partials = reduce_blocks(N);
    hipLaunchKernelGGL(vis_moments1_kernel, dim3(num_partials), dim3(VIS_THREADS), 0, st, depth, N, (int)W, first);
    RNERF_CHECK_LAUNCH();
    hipLaunchKernelGGL(vis_moments2_kernel, dim3(num_partials), dim3(VIS_THREADS), 0, st, depth, N, (int)W, first, second);
    RNERF_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(vis_normals_map_kernel, dim3((unsigned)((N + VIS_THREADS - 1) / VIS_THREADS)), dim3(VIS_THREADS), 0, st, depth, acc, (int)H, (int)W,
                     (float)scaling, second, num_partials, rgb, normals);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}
