// Evaluation metric: SSIM (rnerf/utils.py:404-471, compute_ssim) on the device.
//
// Images are float[n][H][W][C], channels last.  Every leading index and every channel is an independent image; the blur is separable
// (W, then H, "valid"), so in the flat index space of one image row (W*C floats) the horizontal taps of output column j sit at j + k*C:
// the kernel never de-interleaves channels.
//
// One workgroup = one output tile of TH rows x SSIM_TW flat columns of one image.  It loads the tile's TH + fs - 1 input rows of both
// images (each a contiguous segment of a row) into LDS with 16-byte loads, in chunks of RC rows when a whole tile does not fit; the
// horizontal pass writes the five moment planes (x, y, x^2, y^2, xy) into LDS; the vertical pass and the SSIM formula run in registers.
// Every LDS access of both passes is one wave reading or writing 64 consecutive floats (lane = flat column), which is free of bank
// conflicts without padding the rows.
//
// Conditioning: variance and covariance are shift invariant, so each column subtracts a constant (its first input value in the tile, per
// image; 0 when that value is not finite) before squaring.  blur(x^2) - blur(x)^2 then cancels on the scale of the local contrast, not of
// the brightness.  The means mu0 / mu1 are the blurs of the shifted values plus the shift.
//
// The mean is reduced without floating-point atomics: each tile writes one fp64 partial sum; a second launch adds each image's partials
// in a fixed order.  The same inputs give the same bits on every run.
#include "common.h"

#include <math.h>

namespace rnerf {
namespace {

constexpr int SSIM_TW = 64;              // output flat columns per tile: one wave's width
constexpr int SSIM_THREADS = 256;        // 4 waves
constexpr int SSIM_MAX_FS = 31;
constexpr size_t SSIM_LDS_CAP = 64 * 1024;   // <= 64 KiB per workgroup keeps >= 2 workgroups on a CU's 160 KiB

struct SsimFilter { float w[32]; };

struct SsimPlan {
  int rpt;            // output rows per thread in the vertical pass (TH = 4 * rpt)
  int th;             // output rows per tile
  int rows;           // input rows per tile: th + fs - 1
  int rc;             // input rows staged in LDS at a time
  int lin;            // floats per staged input row (16-byte multiple; covers a 3-float alignment lead)
  int tiles_x, tiles_y;
  size_t lds;         // dynamic LDS bytes
};

// LDS layout (floats): [0, 8) four doubles for the workgroup reduction, [8, 40) filter taps, then in0[rc][lin], in1[rc][lin],
// then planes[5][rows][SSIM_TW].
constexpr int SSIM_HDR = 40;

inline bool ssim_plan(int H, int W, int C, int fs, SsimPlan* p) {
  const long long ho = H - fs + 1, wo_flat = (long long)(W - fs + 1) * C;
  const long long lin = ((3 + SSIM_TW + (long long)(fs - 1) * C) + 3) / 4 * 4;
  for (int rpt = 4; rpt >= 1; rpt /= 2) {
    const int th = 4 * rpt, rows = th + fs - 1;
    const long long fixed = SSIM_HDR + 5LL * rows * SSIM_TW;
    const long long avail = (long long)(SSIM_LDS_CAP / 4) - fixed;
    if (avail < 2 * lin) continue;
    const long long rc = avail / (2 * lin) < rows ? avail / (2 * lin) : rows;
    if (rc < rows && rc < 4 && rpt > 1) continue;           // prefer a shorter tile to staging one or two rows at a time
    p->rpt = rpt; p->th = th; p->rows = rows; p->rc = (int)rc; p->lin = (int)lin;
    p->tiles_x = (int)((wo_flat + SSIM_TW - 1) / SSIM_TW);
    p->tiles_y = (int)((ho + th - 1) / th);
    p->lds = (size_t)(fixed + 2 * rc * lin) * 4;
    return true;
  }
  return false;
}

// jnp.minimum / jnp.sign semantics: NaN in -> NaN out (fminf would drop it)
__device__ __forceinline__ float nan_min(float a, float b) { return (a != a || b != b) ? a + b : (a < b ? a : b); }
__device__ __forceinline__ float nan_sign(float a) { return a > 0.f ? 1.f : (a < 0.f ? -1.f : a); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Stage input rows [r0, r0 + rc) of the tile (both images) into LDS rows of `lin` floats.  Row r's segment starts at flat offset g;
// with `vec` the copy starts at the 16-byte boundary below g (lead = g & 3 floats) and moves float4s; a float4 that would pass the end of
// the buffer (`total` floats) is copied element by element.
__device__ __forceinline__ void ssim_stage(const float* __restrict__ img0, const float* __restrict__ img1, float* in0, float* in1,
                                           long long row_base, long long row_stride, int r0, int rc, int cols, int lin, long long total,
                                           bool vec) {
  const int tid = threadIdx.x;
  if (vec) {
    const int nv = lin / 4;
    for (int it = tid; it < rc * nv; it += SSIM_THREADS) {
      const int r = it / nv, q = it - r * nv;
      const long long g = row_base + (long long)(r0 + r) * row_stride;
      const int lead = (int)(g & 3);
      if (4 * q >= lead + cols) continue;
      const long long a = (g - lead) + 4LL * q;
      float4 v0, v1;
      if (a + 4 <= total) {
        v0 = *reinterpret_cast<const float4*>(img0 + a);
        v1 = *reinterpret_cast<const float4*>(img1 + a);
      } else {
        float t0[4], t1[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { t0[e] = a + e < total ? img0[a + e] : 0.f; t1[e] = a + e < total ? img1[a + e] : 0.f; }
        v0 = make_float4(t0[0], t0[1], t0[2], t0[3]); v1 = make_float4(t1[0], t1[1], t1[2], t1[3]);
      }
      *reinterpret_cast<float4*>(in0 + r * lin + 4 * q) = v0;
      *reinterpret_cast<float4*>(in1 + r * lin + 4 * q) = v1;
    }
  } else {                                            // an image pointer that is not 16-byte aligned: plain loads, no lead
    for (int it = tid; it < rc * lin; it += SSIM_THREADS) {
      const int r = it / lin, c = it - r * lin;
      if (c >= cols) continue;
      const long long g = row_base + (long long)(r0 + r) * row_stride + c;
      in0[r * lin + c] = img0[g];
      in1[r * lin + c] = img1[g];
    }
  }
}

template <int RPT>
__global__ __launch_bounds__(SSIM_THREADS) void ssim_tile_kernel(const float* __restrict__ img0, const float* __restrict__ img1, int H, int W,
                                                                 int C, int fs, int rc, int lin, int tiles_x, int tiles_y, SsimFilter filt, float c1,
                                                                 float c2, long long total, int vec, float* __restrict__ map,
                                                                 double* __restrict__ partials) {
  constexpr int TH = 4 * RPT;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  double* red = reinterpret_cast<double*>(lds);
  float* f = lds + 8;
  float* in0 = lds + SSIM_HDR;
  float* in1 = in0 + rc * lin;
  const int rows_max = TH + fs - 1;
  float* planes = in1 + rc * lin;                       // [5][rows_max][SSIM_TW]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long b = blockIdx.x;
  const int tx = (int)(b % tiles_x), ty = (int)((b / tiles_x) % tiles_y);
  const long long img = b / ((long long)tiles_x * tiles_y);
  const int Ho = H - fs + 1, wo_flat = (W - fs + 1) * C;
  const int oy0 = ty * TH, ox0 = tx * SSIM_TW;
  const int nrow = Ho - oy0 < TH ? Ho - oy0 : TH;
  const int ncol = wo_flat - ox0 < SSIM_TW ? wo_flat - ox0 : SSIM_TW;
  const int rows = nrow + fs - 1;                       // input rows this tile reads
  const int cols = ncol + (fs - 1) * C;                 // input floats per row
  const long long row_stride = (long long)W * C;
  const long long row_base = (img * H + oy0) * row_stride + ox0;

#pragma unroll
  for (int k = 0; k < 32; ++k)
    if (tid == k) f[k] = filt.w[k];

  // horizontal pass, chunk by chunk: wave w takes rows w, w+4, ... of the chunk; lane = flat output column
  float sh0 = 0.f, sh1 = 0.f;
  for (int r0 = 0; r0 < rows; r0 += rc) {
    const int n = rows - r0 < rc ? rows - r0 : rc;
    if (r0 > 0) __syncthreads();                        // the previous chunk's readers are done with in0 / in1
    ssim_stage(img0, img1, in0, in1, row_base, row_stride, r0, n, cols, lin, total, vec != 0);
    __syncthreads();
    if (r0 == 0 && lane < ncol) {
      const int lead = vec ? (int)(row_base & 3) : 0;
      const float a = in0[lead + lane], c = in1[lead + lane];
      sh0 = isfinite(a) ? a : 0.f;
      sh1 = isfinite(c) ? c : 0.f;
    }
    if (lane < ncol) {
      for (int r = wave; r < n; r += 4) {
        const long long g = row_base + (long long)(r0 + r) * row_stride;
        const int base = r * lin + (vec ? (int)(g & 3) : 0) + lane;
        float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f, h4 = 0.f;
        for (int k = 0; k < fs; ++k) {
          const float w = f[k];
          const float x = in0[base + k * C] - sh0, y = in1[base + k * C] - sh1;
          const float wx = w * x, wy = w * y;
          h0 += wx; h1 += wy;
          h2 = fmaf(wx, x, h2); h3 = fmaf(wy, y, h3); h4 = fmaf(wx, y, h4);
        }
        const int pr = (r0 + r) * SSIM_TW + lane;
        planes[pr] = h0;
        planes[rows_max * SSIM_TW + pr] = h1;
        planes[2 * rows_max * SSIM_TW + pr] = h2;
        planes[3 * rows_max * SSIM_TW + pr] = h3;
        planes[4 * rows_max * SSIM_TW + pr] = h4;
      }
    }
  }
  __syncthreads();

  // vertical pass: wave w owns output rows [w*RPT, w*RPT + RPT) of column `lane`; each plane row is read once and feeds up to RPT outputs
  double part = 0.0;
  if (lane < ncol) {
    float acc[RPT][5];
#pragma unroll
    for (int q = 0; q < RPT; ++q)
#pragma unroll
      for (int p = 0; p < 5; ++p) acc[q][p] = 0.f;
    const int i0 = wave * RPT;
    for (int r = 0; r < RPT + fs - 1; ++r) {
      const int row = i0 + r;
      if (row >= rows) break;
      float v[5];
#pragma unroll
      for (int p = 0; p < 5; ++p) v[p] = planes[(p * rows_max + row) * SSIM_TW + lane];
#pragma unroll
      for (int q = 0; q < RPT; ++q) {
        const int k = r - q;
        if (k >= 0 && k < fs) {
          const float w = f[k];
#pragma unroll
          for (int p = 0; p < 5; ++p) acc[q][p] = fmaf(w, v[p], acc[q][p]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
      const int i = i0 + q;
      if (i >= nrow) break;
      const float m0 = acc[q][0], m1 = acc[q][1];
      const float mu0 = m0 + sh0, mu1 = m1 + sh1;
      const float mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
      float s00 = acc[q][2] - m0 * m0, s11 = acc[q][3] - m1 * m1, s01 = acc[q][4] - m0 * m1;
      s00 = s00 < 0.f ? 0.f : s00;                      // jnp.maximum(0, s): NaN stays NaN
      s11 = s11 < 0.f ? 0.f : s11;
      s01 = nan_sign(s01) * nan_min(sqrtf(s00 * s11), fabsf(s01));
      const float numer = (2.f * mu01 + c1) * (2.f * s01 + c2);
      const float denom = (mu00 + mu11 + c1) * (s00 + s11 + c2);
      const float m = numer / denom;
      if (map) map[(img * Ho + oy0 + i) * (long long)wo_flat + ox0 + lane] = m;
      part += (double)m;
    }
  }
  if (partials) {
    part = wave_sum(part);
    if (lane == 0) red[wave] = part;
    __syncthreads();
    if (tid == 0) partials[b] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

// one workgroup per image: its tiles' partial sums in a fixed order, divided by the map's size
__global__ __launch_bounds__(SSIM_THREADS) void ssim_mean_kernel(const double* __restrict__ partials, int tiles, double count, float* __restrict__ mean) {
  __shared__ double red[4];
  const long long img = blockIdx.x;
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int t = tid; t < tiles; t += SSIM_THREADS) s += partials[img * tiles + t];
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) mean[img] = (float)((((red[0] + red[1]) + red[2]) + red[3]) / count);
}

int ssim_check(int64_t n, int32_t H, int32_t W, int32_t C, int32_t fs, SsimPlan* p) {
  RNERF_CHECK_ARG(fs >= 1 && fs <= SSIM_MAX_FS, "rnerf_ssim: filter_size must be in [1, %d], got %d", SSIM_MAX_FS, fs);
  RNERF_CHECK_ARG(n >= 1 && C >= 1, "rnerf_ssim: need n >= 1 and C >= 1");
  RNERF_CHECK_ARG(H >= fs && W >= fs, "rnerf_ssim: the image (H %d, W %d) is smaller than the window (filter_size %d)", H, W, fs);
  RNERF_CHECK_ARG((long long)W * C <= (1LL << 30), "rnerf_ssim: W * C too large");
  if (!ssim_plan(H, W, C, fs, p)) {
    set_error("rnerf_ssim: %d channels with filter_size %d need more LDS than a tile may use", C, fs);
    return RNERF_ERR_UNSUPPORTED;
  }
  RNERF_CHECK_ARG((long long)p->tiles_x * p->tiles_y * n <= 0xffffffffLL / SSIM_THREADS, "rnerf_ssim: too many tiles for one launch");
  return RNERF_OK;
}

}  // namespace
}  // namespace rnerf

using namespace rnerf;

extern "C" size_t rnerf_ssim_workspace_bytes(int64_t n, int32_t H, int32_t W, int32_t C, int32_t filter_size) {
  SsimPlan p;
  if (ssim_check(n, H, W, C, filter_size, &p) != RNERF_OK) return 0;
  return (size_t)n * p.tiles_x * p.tiles_y * sizeof(double);
}

extern "C" int rnerf_ssim(const float* img0, const float* img1, int64_t n, int32_t H, int32_t W, int32_t C, int32_t filter_size, double filter_sigma,
                          double max_val, double k1, double k2, float* map, float* mean, void* workspace, void* stream) {
  SsimPlan p;
  const int rc = ssim_check(n, H, W, C, filter_size, &p);
  if (rc != RNERF_OK) return rc;
  RNERF_CHECK_ARG(filter_sigma > 0.0 && isfinite(filter_sigma), "rnerf_ssim: filter_sigma must be finite and > 0");
  RNERF_CHECK_ARG(img0 && img1 && (map || mean), "rnerf_ssim: null pointer (img0, img1, and map or mean)");
  RNERF_CHECK_ARG(!mean || workspace, "rnerf_ssim: the mean needs the workspace (rnerf_ssim_workspace_bytes)");
  RNERF_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "rnerf_ssim: the workspace must be 8-byte aligned");
  // rnerf/utils.py:435-439, in double, rounded once
  const int fs = filter_size, hw = fs / 2;
  const double shift = (2 * hw - fs + 1) / 2.0;
  double w[SSIM_MAX_FS], sum = 0.0;
  for (int i = 0; i < fs; ++i) {
    const double t = (i - hw + shift) / filter_sigma;
    w[i] = exp(-0.5 * t * t);
    sum += w[i];
  }
  RNERF_CHECK_ARG(sum > 0.0 && isfinite(sum), "rnerf_ssim: the filter's weights sum to %g", sum);
  SsimFilter filt = {};
  for (int i = 0; i < fs; ++i) filt.w[i] = (float)(w[i] / sum);
  const float c1 = (float)((k1 * max_val) * (k1 * max_val)), c2 = (float)((k2 * max_val) * (k2 * max_val));
  const long long total = n * H * (long long)W * C;
  const int vec = ((((uintptr_t)img0) | ((uintptr_t)img1)) & 15) == 0;
  const long long tiles = (long long)p.tiles_x * p.tiles_y;
  hipStream_t st = (hipStream_t)stream;
  double* partials = mean ? (double*)workspace : nullptr;
  const dim3 grid((unsigned)(tiles * n)), block(SSIM_THREADS);
#define RNERF_SSIM_LAUNCH(R)                                                                                                              \
  hipLaunchKernelGGL(ssim_tile_kernel<R>, grid, block, p.lds, st, img0, img1, H, W, C, fs, p.rc, p.lin, p.tiles_x, p.tiles_y, filt, c1, c2, \
                     total, vec, map, partials)
  switch (p.rpt) {
    case 4: RNERF_SSIM_LAUNCH(4); break;
    case 2: RNERF_SSIM_LAUNCH(2); break;
    default: RNERF_SSIM_LAUNCH(1); break;
  }
#undef RNERF_SSIM_LAUNCH
  RNERF_CHECK_LAUNCH();
  if (mean) {
    const double count = (double)(H - fs + 1) * (double)(W - fs + 1) * (double)C;
    hipLaunchKernelGGL(ssim_mean_kernel, dim3((unsigned)n), dim3(SSIM_THREADS), 0, st, partials, (int)tiles, count, mean);
    RNERF_CHECK_LAUNCH();
  }
  return RNERF_OK;
}
