// LPIPS on the device: lpips.LPIPS(net='alex'), version 0.1, as metric/summary.py:63-68 calls it (model(ref, src, normalize=True)).
//
// Plan for n image pairs (the 2 n images go through the network as one batch: images 0..n-1 are img0, n..2n-1 are img1):
//   1. lpips_conv_kernel x 5: each convolution as an implicit GEMM on __builtin_amdgcn_mfma_f32_32x32x2f32 (exact fp32: a k-ordered fmaf
//      chain per output), D[cout][pixel] = sum_k W[cout][k] * im2col[k][pixel], k = (ci * KS + ky) * KS + kx in torch's own weight
//      order, so the flat weight buffer is read as it is and nothing is packed.  A workgroup (4 waves) owns 64 couts x 128 pixels of
//      the batch; a wave 64 couts x 32 pixels (two accumulators).  K goes by in chunks of 32: the weight tile [32][64] and the gathered
//      im2col tile [32][128] are staged in LDS (rows padded to an odd length: a wave's 32-lane groups read 32 consecutive floats and
//      write 32 different rows, both without bank conflicts), the next chunk's global loads are in flight while the MFMAs of this one
//      run.  The im2col matrix never exists in memory.  conv1 gathers from the [H][W][3] images and applies the input scaling
//      (2 x - 1, then (x - shift) / scale) to the pixels it reads; the zero padding is of the scaled input, so padding stays 0.
//      Bias and ReLU in the epilogue; activations are planar, float[image][channel][pixel], so a lane's stores and the next layer's
//      gathers run along the pixels.  Tails: pixels >= M and k >= K are gathered as 0, stores are masked; Cout is a multiple of 64.
//   2. lpips_pool_kernel after conv1 and conv2: MaxPool 3 / 2, floor, no padding.
//   3. lpips_tap_kernel after each convolution: per pixel the channel norms of both features, sum_c lin[c] (f0 / (|f0| + 1e-10) -
//      f1 / (|f1| + 1e-10))^2 = d_l, and the fp64 sum of the workgroup's 64 pixels as one partial.  The four waves of a workgroup
//      split the channels and are added in a fixed order.
//   4. lpips_value_kernel: value = sum_l (sum of the partials in a fixed order) / P_l, l = 0..4, in fp64, rounded once.
//      lpips_map_kernel: map = sum_l bilinear(d_l) (align_corners=False), l = 0..4 in float32.
// No atomics anywhere: the same inputs give the same bytes.  Both images of a pair take the same instruction sequence and an output
// element's chain does not depend on where in a tile it sits, so identical images give exactly 0 and swapping them changes nothing.
#include "mfma_ops.h"

namespace rnerf {
namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_BM = 128, LP_BN = 64, LP_BK = 32;          // pixels x couts x k per workgroup and chunk
constexpr int LP_WS = LP_BN + 1, LP_XS = LP_BM + 1;         // LDS row lengths (odd)
constexpr int LP_LAYERS = 5;
constexpr int LP_MIN = 31;                                  // below it the second pool is empty
constexpr int LP_TAP_PIX = 64;                              // pixels per workgroup of the tap kernel
constexpr float LP_EPS = 1e-10f;
constexpr int LP_COUT[LP_LAYERS] = {64, 192, 384, 256, 256};
constexpr int LP_CIN[LP_LAYERS] = {3, 64, 192, 384, 256};
constexpr int LP_KS[LP_LAYERS] = {11, 5, 3, 3, 3};
constexpr size_t LP_WEIGHT_FLOATS = 2470848;

struct LpipsPlan {
  int h[LP_LAYERS], w[LP_LAYERS];       // the taps' sizes
  int hp[2], wp[2];                     // after pool 1 and pool 2
  long long d_off[LP_LAYERS], d_total;  // d_l inside a pair's block of the layer maps
  int blocks[LP_LAYERS];                // tap workgroups (= partials) per pair
  long long part_off[LP_LAYERS], part_total;
  size_t w_off[LP_LAYERS], b_off[LP_LAYERS], lin_off[LP_LAYERS];
  size_t act_off[LP_LAYERS], pool_off[2], d_bytes_off, bytes;       // workspace, in bytes
};

int lpips_plan(int64_t n, int32_t H, int32_t W, LpipsPlan* p) {
  RNERF_CHECK_ARG(n >= 1 && n <= 65535, "rnerf_lpips: need 1 <= n <= 65535");
  RNERF_CHECK_ARG(H >= LP_MIN && W >= LP_MIN, "rnerf_lpips: the images (%d x %d) are smaller than %d x %d, the smallest size AlexNet's second pool accepts", H, W, LP_MIN, LP_MIN);
  p->h[0] = (H - 7) / 4 + 1; p->w[0] = (W - 7) / 4 + 1;
  p->hp[0] = (p->h[0] - 3) / 2 + 1; p->wp[0] = (p->w[0] - 3) / 2 + 1;
  p->h[1] = p->hp[0]; p->w[1] = p->wp[0];
  p->hp[1] = (p->h[1] - 3) / 2 + 1; p->wp[1] = (p->w[1] - 3) / 2 + 1;
  for (int l = 2; l < LP_LAYERS; ++l) { p->h[l] = p->hp[1]; p->w[l] = p->wp[1]; }
  // every kernel indexes with int: the images and the largest activation (conv1's, 64 channels) of the batch must stay below 2^31 floats
  const long long in_floats = 2 * n * (long long)H * W * 3, act0 = 2 * n * 64LL * p->h[0] * p->w[0];
  RNERF_CHECK_ARG(in_floats < (1LL << 31) && act0 < (1LL << 31) && (long long)H * W < (1LL << 31) / 3,
                  "rnerf_lpips: n * H * W too large for the kernels' 32-bit indices");
  size_t wo = 0;
  for (int l = 0; l < LP_LAYERS; ++l) {
    p->w_off[l] = wo; wo += (size_t)LP_COUT[l] * LP_CIN[l] * LP_KS[l] * LP_KS[l];
    p->b_off[l] = wo; wo += LP_COUT[l];
  }
  for (int l = 0; l < LP_LAYERS; ++l) { p->lin_off[l] = wo; wo += LP_COUT[l]; }
  long long d = 0, parts = 0;
  for (int l = 0; l < LP_LAYERS; ++l) {
    const long long P = (long long)p->h[l] * p->w[l];
    p->d_off[l] = d; d += P;
    p->blocks[l] = (int)((P + LP_TAP_PIX - 1) / LP_TAP_PIX);
    p->part_off[l] = parts; parts += p->blocks[l];
  }
  p->d_total = d; p->part_total = parts;
  auto al = [](size_t b) { return (b + 255) / 256 * 256; };
  size_t at = al((size_t)n * parts * sizeof(double));
  for (int l = 0; l < LP_LAYERS; ++l) { p->act_off[l] = at; at += al((size_t)2 * n * LP_COUT[l] * p->h[l] * p->w[l] * sizeof(float)); }
  for (int i = 0; i < 2; ++i) { p->pool_off[i] = at; at += al((size_t)2 * n * LP_COUT[i] * p->hp[i] * p->wp[i] * sizeof(float)); }
  p->d_bytes_off = at; at += al((size_t)n * d * sizeof(float));
  p->bytes = at;
  return RNERF_OK;
}

// ---- the convolutions ----------------------------------------------------------------------------------------------------------------
// FIRST: `in` / `in1` are the n images of each side, float[n][Hi][Wi][3], and Cin = 3; otherwise `in` is float[2n][Cin][Hi][Wi].
template <int KS, int STRIDE, int PAD, bool FIRST>
__global__ __launch_bounds__(LP_THREADS) void lpips_conv_kernel(const float* __restrict__ in, const float* __restrict__ in1, int n_side, int Cin,
                                                                int Hi, int Wi, int Ho, int Wo, int M, int K, const float* __restrict__ wt,
                                                                const float* __restrict__ bias, int Cout, float* __restrict__ out) {
  __shared__ float ws[LP_BK * LP_WS];
  __shared__ float xs[LP_BK * LP_XS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * LP_BM, n0 = blockIdx.y * LP_BN;
  const int P = Ho * Wo;

  // this thread's im2col column: pixel gm of the batch, k = k0 + gk + 2 j
  const int gm = m0 + (tid & (LP_BM - 1)), gk = tid >> 7;
  const bool gvalid = gm < M;
  int iy0 = 0, ix0 = 0;
  const float* __restrict__ src = in;
  if (gvalid) {
    const int b = gm / P, p = gm - b * P, oy = p / Wo, ox = p - oy * Wo;
    iy0 = oy * STRIDE - PAD; ix0 = ox * STRIDE - PAD;
    if constexpr (FIRST) src = b < n_side ? in + b * (Hi * Wi * 3) : in1 + (b - n_side) * (Hi * Wi * 3);
    else src = in + b * (Cin * Hi * Wi);
  }
  auto gather = [&](int k) -> float {
    if (!gvalid || k >= K) return 0.f;
    const int ci = k / (KS * KS), r = k - ci * (KS * KS), ky = r / KS, kx = r - ky * KS;
    const int iy = iy0 + ky, ix = ix0 + kx;
    if (iy < 0 || iy >= Hi || ix < 0 || ix >= Wi) return 0.f;
    if constexpr (FIRST) {
      const float v = src[(iy * Wi + ix) * 3 + ci];
      const float x = fsub(fmul(2.f, v), 1.f);
      const float shift = ci == 0 ? -0.030f : (ci == 1 ? -0.088f : -0.188f), scale = ci == 0 ? 0.458f : (ci == 1 ? 0.448f : 0.450f);
      return fdiv(fsub(x, shift), scale);
    } else {
      return src[(ci * Hi + iy) * Wi + ix];
    }
  };
  // this thread's weights: cout n0 + wc + 8 j, k = k0 + wk
  const int wk = tid & 31, wc = tid >> 5;

  float xr[16], wr[8];
  auto load_chunk = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 16; ++j) xr[j] = gather(k0 + gk + 2 * j);
#pragma unroll
    for (int j = 0; j < 8; ++j) wr[j] = k0 + wk < K ? wt[(n0 + wc + 8 * j) * K + k0 + wk] : 0.f;
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int j = 0; j < 16; ++j) xs[(gk + 2 * j) * LP_XS + (tid & (LP_BM - 1))] = xr[j];
#pragma unroll
    for (int j = 0; j < 8; ++j) ws[wk * LP_WS + wc + 8 * j] = wr[j];
  };

  f32x16 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  const int i = lane & 31, h = lane >> 5;
  const int chunks = (K + LP_BK - 1) / LP_BK;
  load_chunk(0);
  store_chunk();
  __syncthreads();
  for (int c = 0; c < chunks; ++c) {
    if (c + 1 < chunks) load_chunk((c + 1) * LP_BK);
#pragma unroll
    for (int s = 0; s < LP_BK / 2; ++s) {
      const int k = 2 * s + h;
      const float x = xs[k * LP_XS + 32 * wave + i];
      const float a0 = ws[k * LP_WS + i], a1 = ws[k * LP_WS + 32 + i];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, x, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, x, acc[1], 0, 0, 0);
    }
    __syncthreads();
    if (c + 1 < chunks) store_chunk();
    __syncthreads();
  }

  // the lane holds pixel m0 + 32 wave + i and couts n0 + 32 t + (r & 3) + 8 (r >> 2) + 4 h
  const int m = m0 + 32 * wave + i;
  if (m >= M) return;
  const int b = m / P, p = m - b * P;
  float* __restrict__ o = out + (b * Cout + n0) * P + p;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
      const float v = fadd(acc[t][r], bias[n0 + co]);
      o[co * P] = v > 0.f ? v : (v != v ? v : 0.f);          // ReLU; NaN stays NaN as in torch
    }
}

// MaxPool2d(3, 2), floor, no padding, on planes float[planes][Hi][Wi] -> float[planes][Ho][Wo].  NaN propagates as in torch.
__global__ __launch_bounds__(LP_THREADS) void lpips_pool_kernel(const float* __restrict__ in, int planes, int Hi, int Wi, int Ho, int Wo, float* __restrict__ out) {
  const int at = blockIdx.x * LP_THREADS + threadIdx.x;
  const int P = Ho * Wo;
  if (at >= planes * P) return;
  const int pl = at / P, p = at - pl * P, oy = p / Wo, ox = p - oy * Wo;
  const float* __restrict__ s = in + (pl * Hi + 2 * oy) * Wi + 2 * ox;
  float m = s[0];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const float v = s[dy * Wi + dx];
      m = (v > m || v != v) ? v : m;
    }
  out[at] = m;
}

// ---- one tap -------------------------------------------------------------------------------------------------------------------------
// feat: float[2n][C][P].  Workgroup (bx, q): pixels 64 bx .. of pair q; wave w takes the channels w, w + 4, ...  d: this layer's map of
// pair q at d + q * d_stride; partials (nullable): partials[q * part_stride + bx] = the fp64 sum of the workgroup's d.
__global__ __launch_bounds__(LP_THREADS) void lpips_tap_kernel(const float* __restrict__ feat, int n, int C, int P, const float* __restrict__ lin,
                                                               float* __restrict__ d, long long d_stride, double* __restrict__ partials,
                                                               long long part_stride) {
  __shared__ float red[4][LP_TAP_PIX][2];
  __shared__ double sum[LP_TAP_PIX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.y, p = blockIdx.x * LP_TAP_PIX + lane;
  const bool valid = p < P;
  const float* __restrict__ f0 = feat + q * (C * P) + p;
  const float* __restrict__ f1 = feat + (n + q) * (C * P) + p;
  float s0 = 0.f, s1 = 0.f;
  if (valid)
    for (int c = wave; c < C; c += 4) {
      const float a = f0[c * P], b = f1[c * P];
      s0 = fadd(s0, fmul(a, a)); s1 = fadd(s1, fmul(b, b));
    }
  red[wave][lane][0] = s0; red[wave][lane][1] = s1;
  __syncthreads();
  s0 = fadd(fadd(fadd(red[0][lane][0], red[1][lane][0]), red[2][lane][0]), red[3][lane][0]);
  s1 = fadd(fadd(fadd(red[0][lane][1], red[1][lane][1]), red[2][lane][1]), red[3][lane][1]);
  __syncthreads();
  const float r0 = fadd(fsqrt(s0), LP_EPS), r1 = fadd(fsqrt(s1), LP_EPS);
  float acc = 0.f;
  if (valid)
    for (int c = wave; c < C; c += 4) {
      const float df = fsub(fdiv(f0[c * P], r0), fdiv(f1[c * P], r1));
      acc = fadd(acc, fmul(lin[c], fmul(df, df)));
    }
  red[wave][lane][0] = acc;
  __syncthreads();
  if (wave == 0) {
    const float v = fadd(fadd(fadd(red[0][lane][0], red[1][lane][0]), red[2][lane][0]), red[3][lane][0]);
    if (valid) d[q * d_stride + p] = v;
    sum[lane] = valid ? (double)v : 0.0;
  }
  if (!partials) return;
  for (int off = LP_TAP_PIX / 2; off >= 1; off >>= 1) {
    __syncthreads();
    if (tid < off) sum[tid] += sum[tid + off];
  }
  if (tid == 0) partials[q * part_stride + blockIdx.x] = sum[0];
}

struct LpipsLayers {
  int h[LP_LAYERS], w[LP_LAYERS], blocks[LP_LAYERS];
  long long d_off[LP_LAYERS], part_off[LP_LAYERS];
};

// value[q] = sum over l = 0..4 of mean(d_l): the partials of each layer in a fixed order in fp64.  One workgroup per pair.
__global__ __launch_bounds__(LP_THREADS) void lpips_value_kernel(const double* __restrict__ partials, long long part_stride, LpipsLayers L,
                                                                 float* __restrict__ value) {
  __shared__ double red[LP_THREADS];
  const int tid = threadIdx.x, q = blockIdx.x;
  double total = 0.0;
  for (int l = 0; l < LP_LAYERS; ++l) {
    const double* __restrict__ src = partials + q * part_stride + L.part_off[l];
    double s = 0.0;
    for (int t = tid; t < L.blocks[l]; t += LP_THREADS) s += src[t];
    red[tid] = s;
    for (int off = LP_THREADS / 2; off >= 1; off >>= 1) {
      __syncthreads();
      if (tid < off) red[tid] += red[tid + off];
    }
    __syncthreads();
    total += red[0] / ((double)L.h[l] * (double)L.w[l]);
    __syncthreads();
  }
  if (tid == 0) value[q] = (float)total;
}

// torch's upsample_bilinear2d with align_corners=False along one axis: source index, its upper neighbour and the weight of that one
__device__ __forceinline__ void lpips_bilinear_axis(int dst, float scale, int in, int* i0, int* i1, float* l1) {
  float s = fsub(fmul(scale, fadd((float)dst, 0.5f)), 0.5f);
  s = s < 0.f ? 0.f : s;
  int a = (int)s;
  a = a > in - 1 ? in - 1 : a;
  *i0 = a; *i1 = a < in - 1 ? a + 1 : a; *l1 = fsub(s, (float)a);
}

// map[q][y][x] = sum over l = 0..4 of bilinear(d_l)[y][x], in that order in float32.  One thread per pixel.
__global__ __launch_bounds__(LP_THREADS) void lpips_map_kernel(const float* __restrict__ d, long long d_stride, LpipsLayers L, int H, int W,
                                                               float* __restrict__ map) {
  const int at = blockIdx.x * LP_THREADS + threadIdx.x, q = blockIdx.y;
  if (at >= H * W) return;
  const int y = at / W, x = at - y * W;
  float total = 0.f;
#pragma unroll
  for (int l = 0; l < LP_LAYERS; ++l) {
    const int h = L.h[l], w = L.w[l];
    const float* __restrict__ s = d + q * d_stride + L.d_off[l];
    int y0, y1, x0, x1;
    float ly, lx;
    lpips_bilinear_axis(y, (float)h / (float)H, h, &y0, &y1, &ly);
    lpips_bilinear_axis(x, (float)w / (float)W, w, &x0, &x1, &lx);
    const float hy = fsub(1.f, ly), hx = fsub(1.f, lx);
    const float top = fadd(fmul(hx, s[y0 * w + x0]), fmul(lx, s[y0 * w + x1]));
    const float bot = fadd(fmul(hx, s[y1 * w + x0]), fmul(lx, s[y1 * w + x1]));
    total = fadd(total, fadd(fmul(hy, top), fmul(ly, bot)));
  }
  map[(long long)q * H * W + at] = total;
}

template <int KS, int STRIDE, int PAD, bool FIRST>
void launch_conv(const float* in, const float* in1, int n_side, int layer, int Hi, int Wi, int Ho, int Wo, const float* weights, const LpipsPlan& p,
                 float* out, hipStream_t st) {
  const int M = 2 * n_side * Ho * Wo, K = LP_CIN[layer] * KS * KS;
  hipLaunchKernelGGL((lpips_conv_kernel<KS, STRIDE, PAD, FIRST>), dim3((unsigned)((M + LP_BM - 1) / LP_BM), (unsigned)(LP_COUT[layer] / LP_BN)),
                     dim3(LP_THREADS), 0, st, in, in1, n_side, LP_CIN[layer], Hi, Wi, Ho, Wo, M, K, weights + p.w_off[layer],
                     weights + p.b_off[layer], LP_COUT[layer], out);
}

}  // namespace
}  // namespace rnerf

using namespace rnerf;

extern "C" size_t rnerf_lpips_weight_floats(void) { return LP_WEIGHT_FLOATS; }

extern "C" size_t rnerf_lpips_workspace_bytes(int64_t n, int32_t H, int32_t W) {
  LpipsPlan p;
  if (lpips_plan(n, H, W, &p) != RNERF_OK) return 0;
  return p.bytes;
}

extern "C" int rnerf_lpips(const float* img0, const float* img1, int64_t n, int32_t H, int32_t W, const float* weights, float* map, float* value,
                           float* layer_maps, void* workspace, void* stream) {
  LpipsPlan p;
  const int rc = lpips_plan(n, H, W, &p);
  if (rc != RNERF_OK) return rc;
  RNERF_CHECK_ARG(img0 && img1 && weights, "rnerf_lpips: null pointer (img0, img1 or weights)");
  RNERF_CHECK_ARG(map || value || layer_maps, "rnerf_lpips: null pointer (map, value and layer_maps: nothing to compute)");
  RNERF_CHECK_ARG(workspace, "rnerf_lpips: the activations and the partial sums need the workspace (rnerf_lpips_workspace_bytes)");
  RNERF_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "rnerf_lpips: the workspace must be 8-byte aligned");
  static_assert(LP_COUT[0] % LP_BN == 0 && LP_COUT[1] % LP_BN == 0 && LP_COUT[2] % LP_BN == 0 && LP_COUT[3] % LP_BN == 0, "cout tiles");
  hipStream_t st = (hipStream_t)stream;
  char* wsb = (char*)workspace;
  const int nn = (int)n;
  double* partials = value ? (double*)wsb : nullptr;
  float* act[LP_LAYERS];
  for (int l = 0; l < LP_LAYERS; ++l) act[l] = (float*)(wsb + p.act_off[l]);
  float* pool[2] = {(float*)(wsb + p.pool_off[0]), (float*)(wsb + p.pool_off[1])};
  float* d = layer_maps ? layer_maps : (float*)(wsb + p.d_bytes_off);

  auto tap = [&](int l) {
    const int P = p.h[l] * p.w[l];
    hipLaunchKernelGGL(lpips_tap_kernel, dim3((unsigned)p.blocks[l], (unsigned)nn), dim3(LP_THREADS), 0, st, act[l], nn, LP_COUT[l], P,
                       weights + p.lin_off[l], d + p.d_off[l], p.d_total, partials ? partials + p.part_off[l] : nullptr, p.part_total);
  };
  auto pool_launch = [&](int i) {
    const int planes = 2 * nn * LP_COUT[i], total = planes * p.hp[i] * p.wp[i];
    hipLaunchKernelGGL(lpips_pool_kernel, dim3((unsigned)((total + LP_THREADS - 1) / LP_THREADS)), dim3(LP_THREADS), 0, st, act[i], planes, p.h[i], p.w[i],
                       p.hp[i], p.wp[i], pool[i]);
  };
  launch_conv<11, 4, 2, true>(img0, img1, nn, 0, H, W, p.h[0], p.w[0], weights, p, act[0], st);
  RNERF_CHECK_LAUNCH();
  tap(0);
  pool_launch(0);
  RNERF_CHECK_LAUNCH();
  launch_conv<5, 1, 2, false>(pool[0], nullptr, nn, 1, p.hp[0], p.wp[0], p.h[1], p.w[1], weights, p, act[1], st);
  RNERF_CHECK_LAUNCH();
  tap(1);
  pool_launch(1);
  RNERF_CHECK_LAUNCH();
  launch_conv<3, 1, 1, false>(pool[1], nullptr, nn, 2, p.hp[1], p.wp[1], p.h[2], p.w[2], weights, p, act[2], st);
  RNERF_CHECK_LAUNCH();
  tap(2);
  launch_conv<3, 1, 1, false>(act[2], nullptr, nn, 3, p.h[2], p.w[2], p.h[3], p.w[3], weights, p, act[3], st);
  RNERF_CHECK_LAUNCH();
  tap(3);
  launch_conv<3, 1, 1, false>(act[3], nullptr, nn, 4, p.h[3], p.w[3], p.h[4], p.w[4], weights, p, act[4], st);
  RNERF_CHECK_LAUNCH();
  tap(4);
  RNERF_CHECK_LAUNCH();

  LpipsLayers L;
  for (int l = 0; l < LP_LAYERS; ++l) { L.h[l] = p.h[l]; L.w[l] = p.w[l]; L.blocks[l] = p.blocks[l]; L.d_off[l] = p.d_off[l]; L.part_off[l] = p.part_off[l]; }
  if (value) {
    hipLaunchKernelGGL(lpips_value_kernel, dim3((unsigned)nn), dim3(LP_THREADS), 0, st, partials, p.part_total, L, value);
    RNERF_CHECK_LAUNCH();
  }
  if (map) {
    hipLaunchKernelGGL(lpips_map_kernel, dim3((unsigned)((H * W + LP_THREADS - 1) / LP_THREADS), (unsigned)nn), dim3(LP_THREADS), 0, st, d, p.d_total, L, H, W, map);
    RNERF_CHECK_LAUNCH();
  }
  return RNERF_OK;
}
