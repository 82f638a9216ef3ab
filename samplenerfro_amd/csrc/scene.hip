// Ground-truth renderer for synthetic refractive scenes: the eikonal march of a frame's worth of rays that keeps only where each ray ends
// up (rnerf_scene_trace) and the image those rays see in a cube-map environment behind a grey participating medium (rnerf_scene_shade).
// This is the image formation the model family represents (march through the grid, a background that depends on the last bent direction
// only, a medium in front of it) and what the reference's `*_skydome-bkgd_no-partial-reflect_cycles` scenes were rendered with.
// include/rnerf.h has the specification; tests/helpers/scene_ref.py restates the shading in numpy.
//
// The recurrence is march_kernel's (march.hip), restated: the same individually rounded fp32 operations in the same order, so the last
// direction carries the bits rnerf_march writes into path_dr[N-1].  What differs is the launch: a training batch is 4096 rays and its march
// is bound by the latency of one step, hence four lanes per ray, a recorder wave, an LDS ring and corners gathered two steps ahead there.
// A frame is 10^5..10^6 rays and nothing is recorded: the kernel is bound by throughput, eight waves per SIMD cover a gather's latency,
// and one lane per ray issues the fewest instructions per step (profiles/scene/README.md: measured against four lanes per
// ray with and without the speculative gathers).
#include "common.h"

#include <math.h>
#include <stdlib.h>

namespace rnerf {

// What the trace keeps of a ray: node counts against two thresholds.  `inside`: n(p_k) > n_inside.  `refracting`: rnerf_path_summary's
// predicate sqrt_rn((a a + b b) + c c) > eps, evaluated without the square root: sqrt_rn is monotone, so the predicate is `sumsq > ss_max`
// with ss_max the largest float whose correctly rounded root is <= eps (found on the host, scene_ss_max).  A NaN compares false in both.
struct SceneCount { float n_inside, ss_max; };

// One lane per ray: the whole float4 entries of the 8 corners per lane (trilinear_load / trilinear_finish of common.h, the lookup of
// rnerf_grid_query: the operations of march_kernel's quad, one lane doing all four components), no cross-lane traffic, no speculation.
// One wave per workgroup, so that the last waves of a frame spread over the CUs.
__global__ void __launch_bounds__(64) scene_trace_kernel(const float4* __restrict__ table, GridParams g, GridRcp rcp, const float* __restrict__ origins,
                                                              const float* __restrict__ viewdirs, int B, float near, float step, int num_nodes,
                                                              SceneCount cnt, float4* __restrict__ exit_dir, int* __restrict__ counts) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= B) return;
  float dx = viewdirs[3 * (size_t)r], dy = viewdirs[3 * (size_t)r + 1], dz = viewdirs[3 * (size_t)r + 2];
  float px = fadd(origins[3 * (size_t)r], fmul(near, dx)), py = fadd(origins[3 * (size_t)r + 1], fmul(near, dy)), pz = fadd(origins[3 * (size_t)r + 2], fmul(near, dz));
  int n_in = 0, n_refr = 0;
  for (int k = 0;; ++k) {
    TriCell cell;
    trilinear_load<true, true>(table, g, px, py, pz, nullptr, cell, &rcp);
    const float4 c = trilinear_finish(cell);                 // (n, dn/dx, dn/dy, dn/dz)
    n_in += c.x > cnt.n_inside ? 1 : 0;
    n_refr += fadd(fadd(fmul(c.y, c.y), fmul(c.z, c.z)), fmul(c.w, c.w)) > cnt.ss_max ? 1 : 0;
    if (k == num_nodes - 1) break;
    const float s = fdiv(step, c.x);
    px = fadd(px, fmul(s, dx)); py = fadd(py, fmul(s, dy)); pz = fadd(pz, fmul(s, dz));
    dx = fadd(dx, fmul(step, c.y)); dy = fadd(dy, fmul(step, c.z)); dz = fadd(dz, fmul(step, c.w));
  }
  const float nrm = fsqrt(fmaxf(fadd(fadd(fmul(dx, dx), fmul(dy, dy)), fmul(dz, dz)), 1e-6f));
  exit_dir[r] = make_float4(fdiv(dx, nrm), fdiv(dy, nrm), fdiv(dz, nrm), 0.f);
  counts[r] = n_in; counts[(size_t)B + r] = n_refr;
}

#ifdef RNERF_EXPERIMENTS
// ---- four lanes per ray: the forms the one-lane kernel was measured against (librnerf_experiments.so only; tools/scene_time.py --variants,
// profiles/scene/README.md).  march_kernel's marcher wave without the ring: lane q of a quad owns coordinate q of the ray state and component
// (q + 1) & 3 of the table entries.  AHEAD > 0: the corners of step k + AHEAD are gathered from a cell predicted by linear extrapolation
// and gathered again where the prediction was wrong, as in march.hip; AHEAD == 0: every step gathers its own corners and waits for them.
struct SceneGrid {
  int dim[3];
  float nmin[3];
  double rcp_nd[3];        // RN_f64(1 / f32(ndelta))
  unsigned sa[3], sb[3];   // GridParams::sa / sb
};

template <int AHEAD, bool BRICKS>
__global__ void __launch_bounds__(256) scene_trace_quad_kernel(const float* __restrict__ table, SceneGrid g, const float* __restrict__ origins,
                                                               const float* __restrict__ viewdirs, int B, float near, float step, int num_nodes,
                                                               SceneCount cnt, float* __restrict__ exit_dir, int* __restrict__ counts) {
  constexpr int SETS = AHEAD + 1;
  const int q = threadIdx.x & 3;
  const int ray = blockIdx.x * 64 + (threadIdx.x >> 2);
  if (__builtin_amdgcn_readfirstlane(ray) >= B) return;      // the wave's first ray: a whole surplus wave leaves (there is no barrier)
  const bool live = ray < B;
  const int r = live ? ray : B - 1;                           // surplus quads replay the last ray and store nothing
  const int qc = q < 3 ? q : 0;
  const float nmin_q = g.nmin[qc];
  const double rcp_q = g.rcp_nd[qc];
  const int hi_q = g.dim[qc] - 1;
  const unsigned comp = (q + 1) & 3;
  const char* __restrict__ tabc = (const char*)table;
  const unsigned cofs = comp * 4u;
  const unsigned sa_q = g.sa[qc], sb_q = g.sb[qc];
  float d = q < 3 ? viewdirs[3 * (size_t)r + qc] : 0.f;
  float p = q < 3 ? fadd(origins[3 * (size_t)r + qc], fmul(near, d)) : 0.f;

  struct Corners { float c[8]; int i0, i1; };
  Corners cs[SETS];
  auto gather = [&](int i0, int i1, Corners& o) {
    o.i0 = i0; o.i1 = i1;
    unsigned m0, m1;
    if constexpr (BRICKS) {
      m0 = __umul24((unsigned)i0 >> 1, sa_q) + __umul24((unsigned)i0 & 1u, sb_q);
      m1 = __umul24((unsigned)i1 >> 1, sa_q) + __umul24((unsigned)i1 & 1u, sb_q);
    } else {
      m0 = __umul24((unsigned)i0, sb_q); m1 = __umul24((unsigned)i1, sb_q);
    }
    const unsigned y0 = quad_bcast_i<1>(m0), y1 = quad_bcast_i<1>(m1);
    const unsigned z0 = quad_bcast_i<2>(m0) + cofs, z1 = quad_bcast_i<2>(m1) + cofs;
    const unsigned b00 = quad_bcast_i<0>(m0) + y0, b10 = quad_bcast_i<0>(m1) + y0, b01 = quad_bcast_i<0>(m0) + y1, b11 = quad_bcast_i<0>(m1) + y1;
    o.c[0] = *(const float*)(tabc + (b00 + z0)); o.c[1] = *(const float*)(tabc + (b10 + z0));
    o.c[2] = *(const float*)(tabc + (b00 + z1)); o.c[3] = *(const float*)(tabc + (b10 + z1));
    o.c[4] = *(const float*)(tabc + (b01 + z0)); o.c[5] = *(const float*)(tabc + (b11 + z0));
    o.c[6] = *(const float*)(tabc + (b01 + z1)); o.c[7] = *(const float*)(tabc + (b11 + z1));
  };
  auto predict = [&](float xp, Corners& o) {
    const int j = floor_to_int(xp);
    gather(clamp0(j, hi_q), clamp0(j + 1, hi_q), o);
  };
  float x_prev = 0.f;
  if constexpr (AHEAD > 0) {
    const float x = div_const(fsub(p, nmin_q), rcp_q);
    x_prev = div_const(fsub(fsub(p, fmul(step, d)), nmin_q), rcp_q);
    const float dx0 = fsub(x, x_prev);
#pragma unroll
    for (int j = 0; j < AHEAD; ++j) predict(fadd(x, fmul((float)j, dx0)), cs[j]);
  }
  int n_in = 0, n_refr = 0;
  float d_exit = d;
  auto one_step = [&](int k, Corners& cn, Corners& nx) {
    const float x = div_const(fsub(p, nmin_q), rcp_q);
    const float fx = floorf(x);
    const int i = (int)fx;
    const float t = fsub(x, fx);
    const int i0 = clamp0(i, hi_q), i1 = clamp0(i + 1, hi_q);
    if constexpr (AHEAD > 0) {
      if (__builtin_amdgcn_ballot_w64(i0 != cn.i0 || i1 != cn.i1) != 0) gather(i0, i1, cn);
      const float dx = fsub(x, x_prev);
      predict(fadd(x, fmul((float)AHEAD, dx)), nx);
      x_prev = x;
    } else {
      gather(i0, i1, cn);
    }
    const float xd = quad_bcast<0>(t), yd = quad_bcast<1>(t), zd = quad_bcast<2>(t);
    const f32x2_t wx = {fsub(1.0f, xd), xd}, wy = {fsub(1.0f, yd), yd}, wz = {fsub(1.0f, zd), zd};
    const float c00 = lerp_pk(cn.c[0], cn.c[1], wx);
    const float c01 = lerp_pk(cn.c[2], cn.c[3], wx);
    const float c10 = lerp_pk(cn.c[4], cn.c[5], wx);
    const float c11 = lerp_pk(cn.c[6], cn.c[7], wx);
    const float c0 = lerp_pk(c00, c10, wy);
    const float c1 = lerp_pk(c01, c11, wy);
    const float c = lerp_pk(c0, c1, wz);      // lanes 0..2: grad component q, lane 3: n
    const float n = quad_bcast<3>(c);
    if (k < num_nodes) {                      // surplus steps of the last trip: clamped gathers, nothing counted
      n_in += n > cnt.n_inside ? 1 : 0;
      n_refr += quad_sumsq3(c) > cnt.ss_max ? 1 : 0;
    }
    if (k == num_nodes - 1) d_exit = d;       // node N-1 = the state before step N-1
    const float s = fdiv(step, n);
    p = fadd(p, fmul(s, d));
    d = fadd(d, fmul(step, c));
  };
  const int trips = (num_nodes + SETS - 1) / SETS;
  for (int t = 0, k = 0; t < trips; ++t, k += SETS) {      // the corner register sets rotate instead of being copied
#pragma unroll
    for (int u = 0; u < SETS; ++u) one_step(k + u, cs[u], cs[(u + AHEAD) % SETS]);
  }
  const float nrm = fsqrt(fmaxf(quad_sumsq3(d_exit), 1e-6f));
  if (live) {
    exit_dir[4 * (size_t)r + q] = q < 3 ? fdiv(d_exit, nrm) : 0.f;
    if (q == 0) { counts[r] = n_in; counts[(size_t)B + r] = n_refr; }
  }
}
#endif  // RNERF_EXPERIMENTS

// ---- shading --------------------------------------------------------------------------------------------------------------------------------
struct SceneShade { int H, W, K, E; double neg_tau; float albedo[3]; float rcp_kk; };      // neg_tau = (-sigma) * step_len

// a * (1 - w) + b * w, every operation rounded
__device__ __forceinline__ float mix1(float a, float b, float omw, float w) { return fadd(fmul(a, omw), fmul(b, w)); }

// texel coordinate of a face coordinate s in [-1, 1]: u = ((s + 1) * 0.5) * E - 0.5 clamped to [0, E - 1]; i0 = floor, i1 = min(i0 + 1, E - 1)
__device__ __forceinline__ void cube_axis(float s, int E, int& i0, int& i1, float& w) {
  float u = fsub(fmul(fmul(fadd(s, 1.0f), 0.5f), (float)E), 0.5f);
  u = fminf(fmaxf(u, 0.0f), (float)(E - 1));
  const float f = floorf(u);
  i0 = (int)f;
  i1 = i0 + 1 < E ? i0 + 1 : E - 1;
  w = fsub(u, f);
}

// env[face][v][u][3] seen in direction d (include/rnerf.h: rnerf_scene_shade); black for the zero vector, a direction with a NaN component
// and one whose face coordinate is a NaN (inf / inf: two infinite components)
__device__ __forceinline__ void cube_lookup(const float* __restrict__ env, int E, float x, float y, float z, float rgb[3]) {
  const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
  rgb[0] = rgb[1] = rgb[2] = 0.f;
  if (!(ax == ax && ay == ay && az == az)) return;          // a NaN component
  int axis; float m, a, b, major;
  if (ax >= ay && ax >= az) { axis = 0; m = ax; major = x; a = y; b = z; }
  else if (ay >= az) { axis = 1; m = ay; major = y; a = z; b = x; }
  else { axis = 2; m = az; major = z; a = x; b = y; }
  if (!(m > 0.f)) return;
  const int face = 2 * axis + (major < 0.f ? 1 : 0);
  int u0, u1, v0, v1; float wu, wv;
  const float fs = fdiv(a, m), ft = fdiv(b, m);
  if (!(fs == fs && ft == ft)) return;
  cube_axis(fs, E, u0, u1, wu);
  cube_axis(ft, E, v0, v1, wv);
  const float omu = fsub(1.0f, wu), omv = fsub(1.0f, wv);
  const float* __restrict__ f = env + (size_t)face * E * E * 3;
  const float* r0 = f + (size_t)v0 * E * 3;
  const float* r1 = f + (size_t)v1 * E * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float top = mix1(r0[3 * u0 + c], r0[3 * u1 + c], omu, wu);
    const float bot = mix1(r1[3 * u0 + c], r1[3 * u1 + c], omu, wu);
    rgb[c] = mix1(top, bot, omv, wv);
  }
}

// One thread per output pixel; its K x K sub-samples in ascending (row, column) order of the fine image.  No atomics.
__global__ void __launch_bounds__(256) scene_shade_kernel(const float4* __restrict__ exit_dir, const int* __restrict__ counts, SceneShade s,
                                                          const float* __restrict__ env, float* __restrict__ rgb, float* __restrict__ trans,
                                                          unsigned char* __restrict__ mask) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= s.H * s.W) return;
  const int y = pix / s.W, x = pix - y * s.W;
  const size_t fw = (size_t)s.W * s.K, nfine = fw * ((size_t)s.H * s.K);
  float acc[3] = {0.f, 0.f, 0.f}, acc_t = 0.f;
  bool any = false;
  for (int sy = 0; sy < s.K; ++sy) {
    for (int sx = 0; sx < s.K; ++sx) {
      const size_t i = ((size_t)y * s.K + sy) * fw + ((size_t)x * s.K + sx);
      const float4 d = exit_dir[i];
      const int n_in = counts[i];
      any = any || counts[nfine + i] > 0;
      float e[3];
      cube_lookup(env, s.E, d.x, d.y, d.z, e);
      const float T = (float)exp(__dmul_rn(s.neg_tau, (double)n_in));
      const float omT = fsub(1.0f, T);
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = fadd(acc[c], fadd(fmul(T, e[c]), fmul(omT, s.albedo[c])));
      acc_t = fadd(acc_t, T);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) rgb[3 * (size_t)pix + c] = fmul(acc[c], s.rcp_kk);
  trans[pix] = fmul(acc_t, s.rcp_kk);
  mask[pix] = any ? 255 : 0;
}

// the largest float whose correctly rounded square root is <= eps (the host's sqrtf is correctly rounded): sqrt_rn(v) > eps  <=>  v > this
static float scene_ss_max(float eps) {
  if (eps < 0.f) return -1.0f;                       // every sum of squares that is not a NaN passes
  if (isinf(eps)) return eps;
  float c = (float)((double)eps * (double)eps);     // within an ulp or two of the answer; walk to it
  if (isinf(c)) c = 3.402823466e+38f;
  while (sqrtf(c) <= eps && c < 3.402823466e+38f) c = nextafterf(c, INFINITY);
  while (sqrtf(c) > eps) c = nextafterf(c, -INFINITY);
  return c;
}

}  // namespace rnerf

using namespace rnerf;

extern "C" int rnerf_scene_trace(const float* table, const rnerf_grid* g, const float* origins, const float* viewdirs, int32_t B, double near,
                                 double far, int32_t num_nodes, double n_inside, double grad_eps, float* exit_dir, int32_t* counts, void* stream) {
  RNERF_CHECK_ARG(table && g && origins && viewdirs && exit_dir && counts, "rnerf_scene_trace: null pointer");
  RNERF_CHECK_ARG(B >= 1 && num_nodes >= 2, "rnerf_scene_trace: need B >= 1 and num_nodes >= 2");
  RNERF_CHECK_ARG(!isnan(n_inside) && !isnan(grad_eps), "rnerf_scene_trace: n_inside and grad_eps must not be NaN");
  RNERF_CHECK_ARG((((uintptr_t)table | (uintptr_t)exit_dir) & 15) == 0 && ((uintptr_t)counts & 3) == 0,
                  "rnerf_scene_trace: table and exit_dir must be 16-byte aligned, counts 4-byte aligned");
  GridParams gp;
  RNERF_CHECK_ARG(make_grid_params(g, &gp), "rnerf_scene_trace: bad grid");
  RNERF_CHECK_ARG(grid_fits_march(gp), "rnerf_scene_trace: grid too large for 32-bit byte offsets (the limits of rnerf_march)");
  const GridRcp rcp{1.0 / (double)gp.ndx, 1.0 / (double)gp.ndy, 1.0 / (double)gp.ndz};      // as rnerf_march's MarchParams::rcp_nd
  const float stepf = (float)((far - near) / (num_nodes - 1));      // models.py:122, as rnerf_march
  const float nearf = (float)near;
  const SceneCount cnt{(float)n_inside, scene_ss_max((float)grad_eps)};
  const dim3 grid((unsigned)(((int64_t)B + 63) / 64));
  hipStream_t st = (hipStream_t)stream;
#ifdef RNERF_EXPERIMENTS
  // RNERF_SCENE_VARIANT = 4: four lanes per ray, corners gathered two steps ahead; 40: four lanes, no speculation; else the product kernel
  const char* e = RNERF_ENV("RNERF_SCENE_VARIANT");
  const int variant = e ? atoi(e) : 1;
  if (variant == 4 || variant == 40) {
    SceneGrid sg;
    sg.dim[0] = gp.dx; sg.dim[1] = gp.dy; sg.dim[2] = gp.dz;
    sg.nmin[0] = gp.nminx; sg.nmin[1] = gp.nminy; sg.nmin[2] = gp.nminz;
    sg.rcp_nd[0] = rcp.x; sg.rcp_nd[1] = rcp.y; sg.rcp_nd[2] = rcp.z;
    for (int i = 0; i < 3; ++i) { sg.sa[i] = gp.sa[i]; sg.sb[i] = gp.sb[i]; }
    const bool bricks = gp.layout == RNERF_TABLE_BRICKS;
#define SCENE_QUAD(A, K)                                                                                                                    \
  hipLaunchKernelGGL((scene_trace_quad_kernel<A, K>), grid, dim3(256), 0, st, table, sg, origins, viewdirs, B, nearf, stepf, num_nodes, cnt, \
                     exit_dir, counts)
    if (variant == 4) { if (bricks) SCENE_QUAD(2, true); else SCENE_QUAD(2, false); }
    else { if (bricks) SCENE_QUAD(0, true); else SCENE_QUAD(0, false); }
#undef SCENE_QUAD
    RNERF_CHECK_LAUNCH();
    return RNERF_OK;
  }
#endif
  hipLaunchKernelGGL(scene_trace_kernel, grid, dim3(64), 0, st, (const float4*)table, gp, rcp, origins, viewdirs, B, nearf, stepf, num_nodes, cnt,
                     (float4*)exit_dir, counts);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_scene_shade(const float* exit_dir, const int32_t* counts, int32_t H, int32_t W, int32_t K, const float* env, int32_t E,
                                 double step_len, double sigma, const double* albedo, float* rgb, float* trans, uint8_t* mask, void* stream) {
  RNERF_CHECK_ARG(exit_dir && counts && env && albedo && rgb && trans && mask, "rnerf_scene_shade: null pointer");
  RNERF_CHECK_ARG(H >= 1 && W >= 1 && K >= 1 && E >= 1, "rnerf_scene_shade: need H, W, K, E >= 1");
  RNERF_CHECK_ARG((int64_t)H * K <= 2147483647 && (int64_t)W * K <= 2147483647 && (int64_t)H * K * ((int64_t)W * K) <= 2147483647,
                  "rnerf_scene_shade: H K W K must fit int32");
  RNERF_CHECK_ARG(((uintptr_t)exit_dir & 15) == 0, "rnerf_scene_shade: exit_dir must be 16-byte aligned");
  SceneShade s;
  s.H = H; s.W = W; s.K = K; s.E = E;
  s.neg_tau = (-sigma) * step_len;
  for (int c = 0; c < 3; ++c) s.albedo[c] = (float)albedo[c];
  s.rcp_kk = (float)(1.0 / (double)((int64_t)K * K));
  const int64_t npix = (int64_t)H * W;
  hipLaunchKernelGGL(scene_shade_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)exit_dir, counts, s,
                     env, rgb, trans, mask);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}
