// Evaluation metrics on the device: SSIM (rnerf/utils.py:404-471, compute_ssim) and LDR-FLIP (metric/flip/flip_api.py:134-495,
// compute_ldrflip; the FLIP kernels and their plan are described where they start, below the SSIM kernels).
//
// SSIM.
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
//
// The same tile kernel, instantiated with SUMMARY, is metric/summary.py's SSIM (metric/ssim/ssim.py:45-133, rnerf_ssim_summary): only the
// formula after the vertical pass differs.  Its per-channel map goes to the workspace and channel_mean_kernel averages the channels.
// summary.py's squared-error map (rnerf_errmap_mse) is here too, for the fixed-order mean it shares with the other two.
#include "common.h"
#include "eval_host.h"

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

// The tail of every fixed-order fp64 sum here, for a workgroup of four waves: each wave adds its lanes (the xor butterfly above), lane 0
// leaves the wave's sum in red[wave], and the result is ((red[0] + red[1]) + red[2]) + red[3], which thread 0 stores.  The order of
// these additions is the contract: the sums are bit-reproducible.  Every thread of the workgroup must call it.
__device__ __forceinline__ double block_sum4(double v, double* red) {
  const int tid = threadIdx.x;
  v = wave_sum(v);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
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

// SUMMARY: metric/ssim/ssim.py:69-81 instead of rnerf/utils.py:455-469 — the same blurred moments, the variances and the covariance neither
// clamped nor bounded by sign * min, luminance term times contrast-structure term.
template <int RPT, bool SUMMARY>
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
      float m;
      if constexpr (SUMMARY) {
        const float cs = (2.f * s01 + c2) / (s00 + s11 + c2);
        m = ((2.f * mu01 + c1) / (mu00 + mu11 + c1)) * cs;
      } else {
        s00 = s00 < 0.f ? 0.f : s00;                      // jnp.maximum(0, s): NaN stays NaN
        s11 = s11 < 0.f ? 0.f : s11;
        s01 = nan_sign(s01) * nan_min(sqrtf(s00 * s11), fabsf(s01));
        const float numer = (2.f * mu01 + c1) * (2.f * s01 + c2);
        const float denom = (mu00 + mu11 + c1) * (s00 + s11 + c2);
        m = numer / denom;
      }
      if (map) map[(img * Ho + oy0 + i) * (long long)wo_flat + ox0 + lane] = m;
      part += (double)m;
    }
  }
  if (partials) {
    part = block_sum4(part, red);
    if (tid == 0) partials[b] = part;
  }
}

// one workgroup per image: its tiles' partial sums in a fixed order, divided by the map's size
__global__ __launch_bounds__(SSIM_THREADS) void ssim_mean_kernel(const double* __restrict__ partials, int tiles, double count, float* __restrict__ mean) {
  __shared__ double red[4];
  const long long img = blockIdx.x;
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int t = tid; t < tiles; t += SSIM_THREADS) s += partials[img * tiles + t];
  s = block_sum4(s, red);
  if (tid == 0) mean[img] = (float)(s / count);
}

// The channel mean of a per-channel map float[rows][C] -> float[rows] (ssim_map.mean(1), ssim.py:129): the channels added in order in
// float32, divided by C.  One thread per pixel.
__global__ __launch_bounds__(SSIM_THREADS) void channel_mean_kernel(const float* __restrict__ per_channel, long long pixels, int C, float* __restrict__ map) {
  const long long px = (long long)blockIdx.x * SSIM_THREADS + threadIdx.x;
  if (px >= pixels) return;
  float s = per_channel[px * C];
  for (int c = 1; c < C; ++c) s += per_channel[px * C + c];
  map[px] = s / (float)C;
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

// The fs taps exp(exponent(i)) / sum, in double, rounded once.  -> the sum: the taps are set only if it is positive and finite.
template <class Exponent>
double ssim_taps(int fs, Exponent exponent, SsimFilter* filt) {
  double w[SSIM_MAX_FS], sum = 0.0;
  for (int i = 0; i < fs; ++i) {
    w[i] = exp(exponent(i));
    sum += w[i];
  }
  *filt = {};
  if (sum > 0.0 && isfinite(sum))
    for (int i = 0; i < fs; ++i) filt->w[i] = (float)(w[i] / sum);
  return sum;
}

// The tile launch of rnerf_ssim (map: [n][Ho][Wo][C]) and, with SUMMARY, of rnerf_ssim_summary (map: its per-channel map); either of map
// and partials (one double per tile) may be null.
template <bool SUMMARY>
int ssim_launch(const SsimPlan& p, const SsimFilter& filt, float c1, float c2, const float* img0, const float* img1, int64_t n, int H, int W,
                int C, int fs, float* map, double* partials, hipStream_t st) {
  const long long total = n * H * (long long)W * C;
  const int vec = ((((uintptr_t)img0) | ((uintptr_t)img1)) & 15) == 0;
  const dim3 grid((unsigned)((long long)p.tiles_x * p.tiles_y * n)), block(SSIM_THREADS);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, p.lds, st, img0, img1, H, W, C, fs, p.rc, p.lin, p.tiles_x, p.tiles_y, filt, c1, c2, total, vec, map,
                       partials);
  };
  switch (p.rpt) {
    case 4: launch(ssim_tile_kernel<4, SUMMARY>); break;
    case 2: launch(ssim_tile_kernel<2, SUMMARY>); break;
    default: launch(ssim_tile_kernel<1, SUMMARY>); break;
  }
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

// ---- The squared-error map of metric/summary.py:49-54 (rnerf_errmap_mse) -------------------------------------------------------------
//
// One thread per pixel: map = mean over the channels of (ref - test)^2, each operation one rounded float32 operation, the channels
// added in order (torch.mean(..., axis=0) over a few channels).  A workgroup covers 256 consecutive pixels of ONE image; its partial is
// the fp64 sum of the float32 squares.
__global__ __launch_bounds__(SSIM_THREADS) void errmap_mse_kernel(const float* __restrict__ ref, const float* __restrict__ test, long long hw,
                                                                    int C, int blocks_per_image, float* __restrict__ map,
                                                                    double* __restrict__ partials) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const long long blk = blockIdx.x;
  const long long img = blk / blocks_per_image;
  const long long px = (blk - img * blocks_per_image) * SSIM_THREADS + tid;
  double part = 0.0;
  if (px < hw) {
    const long long at = (img * hw + px) * C;
    float sum = 0.f;
    for (int c = 0; c < C; ++c) {
      const float d = fsub(ref[at + c], test[at + c]);
      const float sq = fmul(d, d);
      sum = c == 0 ? sq : fadd(sum, sq);
      part += (double)sq;
    }
    if (map) map[img * hw + px] = fdiv(sum, (float)C);
  }
  if (partials) {
    part = block_sum4(part, red);
    if (tid == 0) partials[blk] = part;
  }
}

int errmap_mse_check(int64_t n, int32_t H, int32_t W, int32_t C, long long* blocks_per_image) {
  RNERF_CHECK_ARG(n >= 1 && H >= 1 && W >= 1 && C >= 1, "rnerf_errmap_mse: need n >= 1, H >= 1, W >= 1 and C >= 1");
  const long long hw = (long long)H * W;
  *blocks_per_image = (hw + SSIM_THREADS - 1) / SSIM_THREADS;
  RNERF_CHECK_ARG(*blocks_per_image <= 0x7fffffffLL / n, "rnerf_errmap_mse: n * H * W too large for one launch");
  RNERF_CHECK_ARG(C <= (1LL << 40) / hw / n, "rnerf_errmap_mse: n * H * W * C too large");
  return RNERF_OK;
}


// ---- LDR-FLIP (metric/flip/flip_api.py:439-495, compute_ldrflip) ------------------------------------------------------------------
//
// Every 2-D filter of the metric is a product of two 1-D vectors or a sum of two such products (the CSFs of A and RG are one Gaussian,
// BY is two; the edge detector is (-x g(x)) g(y), the point detector ((x^2/sd^2 - 1) g(x)) g(y), both normalised per sign, which depends
// on x only), and replicating the border of the image is clamping the row and the column index independently.  So the metric runs as
//   1. flip_horizontal_kernel: a workgroup takes FLIP_HROWS rows x FLIP_HW columns.  It converts the segment and its halo (column index
//      clamped) of both images sRGB -> linear -> XYZ -> YCxCz into LDS (Y, Cx, Cz and the normalised Y of the feature pipeline), and
//      writes seven horizontally filtered planes per image into the workspace: A, RG, the two Gaussians of BY, and the normalised Y under
//      g, under the edge vector and under the point vector;
//   2. flip_vertical_kernel: a workgroup takes FLIP_TH rows x 64 columns; wave w owns FLIP_RPT rows of column `lane`, reads each plane
//      row once (row index clamped; a wave reads 64 consecutive floats), accumulates the vertical taps in registers and runs the
//      pointwise tail: opponent -> linear RGB, clipped -> L*a*b* -> Hunt -> HyAB, ^0.7, redistribution; feature difference; the error;
//   3. ssim_mean_kernel over the tiles' fp64 partials, as for SSIM.
// The 14 planes of an 800 x 800 pair are 36 MB: written and read once, out of the Infinity Cache.  The conversion is repeated only on the
// halo columns (2 r of FLIP_HW + 2 r).  Both images go through one instruction sequence (every per-image step is a loop over the two
// images around the same code), so where the two images agree on a pixel's whole footprint the map is exactly 0.
constexpr int FLIP_MAX_R = 15;
constexpr int FLIP_TAPS = 2 * FLIP_MAX_R + 1;
constexpr int FLIP_THREADS = 256;
constexpr int FLIP_HW = 128, FLIP_HROWS = 2;        // horizontal pass: 2 rows x 128 columns per workgroup
constexpr int FLIP_TW = 64, FLIP_RPT = 4;           // vertical pass: 4 waves x 4 rows x 64 columns
constexpr int FLIP_TH = 4 * FLIP_RPT;
constexpr int FLIP_PLANES = 14;                     // 7 per image: A, RG, BY1, BY2, Yn*g, Yn*edge, Yn*point (horizontal pass only)

// 1-D filter vectors, index k = offset + radius.  a, rg, b1, b2, g sum to 1; vb1 / vb2 are b1 / b2 scaled by the share of each Gaussian
// in the 2-D BY filter's sum; e and p are normalised per sign.  Spatial vectors have 2 rs + 1 taps, feature vectors 2 rf + 1.
struct FlipFilter { float a[FLIP_TAPS], rg[FLIP_TAPS], b1[FLIP_TAPS], b2[FLIP_TAPS], vb1[FLIP_TAPS], vb2[FLIP_TAPS], g[FLIP_TAPS], e[FLIP_TAPS], p[FLIP_TAPS]; };

struct FlipPlan {
  int rs, rf;                  // spatial and feature radius
  int segs, rowblks;           // horizontal pass: workgroups per row, per image column
  int tiles_x, tiles_y;        // vertical pass
};

// linear RGB <-> XYZ (D65) and the reference white, as float32 (the reference rounds them so)
constexpr float FLIP_A11 = (float)(10135552.0 / 24577794.0), FLIP_A12 = (float)(8788810.0 / 24577794.0), FLIP_A13 = (float)(4435075.0 / 24577794.0);
constexpr float FLIP_A21 = (float)(2613072.0 / 12288897.0), FLIP_A22 = (float)(8788810.0 / 12288897.0), FLIP_A23 = (float)(887015.0 / 12288897.0);
constexpr float FLIP_A31 = (float)(1425312.0 / 73733382.0), FLIP_A32 = (float)(8788810.0 / 73733382.0), FLIP_A33 = (float)(70074185.0 / 73733382.0);
constexpr float FLIP_B11 = 3.241003275f, FLIP_B12 = -1.537398934f, FLIP_B13 = -0.498615861f;
constexpr float FLIP_B21 = -0.969224334f, FLIP_B22 = 1.875930071f, FLIP_B23 = 0.041554224f;
constexpr float FLIP_B31 = 0.055639423f, FLIP_B32 = -0.204011202f, FLIP_B33 = 1.057148933f;
constexpr float FLIP_WX = 0.950428545f, FLIP_WZ = 1.088900371f, FLIP_IWX = 1.052156925f, FLIP_IWZ = 0.918357670f;

__device__ __forceinline__ float flip_srgb_to_linear(float c) { return c > 0.04045f ? powf((c + 0.055f) / 1.055f, 2.4f) : c / 12.92f; }

// sRGB -> YCxCz, and the feature pipeline's (Y + 16) / 116
__device__ __forceinline__ void flip_opponent(float r, float g, float b, float* Y, float* cx, float* cz, float* yn) {
  r = flip_srgb_to_linear(r); g = flip_srgb_to_linear(g); b = flip_srgb_to_linear(b);
  const float x = ((FLIP_A11 * r + FLIP_A12 * g) + FLIP_A13 * b) * FLIP_IWX;
  const float y = (FLIP_A21 * r + FLIP_A22 * g) + FLIP_A23 * b;
  const float z = ((FLIP_A31 * r + FLIP_A32 * g) + FLIP_A33 * b) * FLIP_IWZ;
  *Y = 116.f * y - 16.f;
  *cx = 500.f * (x - y);
  *cz = 200.f * (y - z);
  *yn = (*Y + 16.f) / 116.f;
}

__device__ __forceinline__ float flip_clip01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }   // np.clip: NaN stays NaN
__device__ __forceinline__ float flip_lab_f(float t) {
  constexpr float d = 6.f / 29.f;
  return t > d * d * d ? cbrtf(t) : (1.f / (3.f * d * d)) * t + 4.f / 29.f;
}

// filtered YCxCz -> linear RGB, clipped to the unit cube -> L*a*b* -> Hunt-adjusted L*a*b*
__device__ __forceinline__ void flip_hunt_lab(float Y, float cx, float cz, float* L, float* A, float* B) {
  const float fy = (Y + 16.f) / 116.f;
  const float x = (fy + cx / 500.f) * FLIP_WX, y = fy, z = (fy - cz / 200.f) * FLIP_WZ;
  const float r = flip_clip01((FLIP_B11 * x + FLIP_B12 * y) + FLIP_B13 * z);
  const float g = flip_clip01((FLIP_B21 * x + FLIP_B22 * y) + FLIP_B23 * z);
  const float b = flip_clip01((FLIP_B31 * x + FLIP_B32 * y) + FLIP_B33 * z);
  const float lx = flip_lab_f(((FLIP_A11 * r + FLIP_A12 * g) + FLIP_A13 * b) * FLIP_IWX);
  const float ly = flip_lab_f((FLIP_A21 * r + FLIP_A22 * g) + FLIP_A23 * b);
  const float lz = flip_lab_f(((FLIP_A31 * r + FLIP_A32 * g) + FLIP_A33 * b) * FLIP_IWZ);
  const float l = 116.f * ly - 16.f;
  *L = l;
  *A = (0.01f * l) * (500.f * (lx - ly));
  *B = (0.01f * l) * (200.f * (ly - lz));
}

__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }

__global__ __launch_bounds__(FLIP_THREADS) void flip_horizontal_kernel(const float* __restrict__ ref, const float* __restrict__ tst, int H, int W,
                                                                       int rs, int rf, int segs, int rowblks, FlipFilter filt,
                                                                       float* __restrict__ planes, long long plane_stride) {
  constexpr int SPAN = FLIP_HW + 2 * FLIP_MAX_R;
  __shared__ float s[2][FLIP_HROWS][4][SPAN];            // [image][row][Y, Cx, Cz, Yn][column]: a wave reads 64 consecutive floats
  const int tid = threadIdx.x;
  const long long blk = blockIdx.x;
  const int seg = (int)(blk % segs), rb = (int)((blk / segs) % rowblks);
  const long long img = blk / ((long long)segs * rowblks);
  const int x0 = seg * FLIP_HW, y0 = rb * FLIP_HROWS;
  const int ncol = W - x0 < FLIP_HW ? W - x0 : FLIP_HW;
  const int span = ncol + 2 * rs;
  for (int it = tid; it < FLIP_HROWS * span; it += FLIP_THREADS) {
    const int rr = it / span, c = it - rr * span;
    const int y = y0 + rr;
    if (y >= H) continue;
    int x = x0 + c - rs;
    x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
    const long long at = ((img * H + y) * W + x) * 3;
#pragma unroll
    for (int im = 0; im < 2; ++im) {
      const float* __restrict__ src = im == 0 ? ref : tst;
      float Y, cx, cz, yn;
      flip_opponent(src[at], src[at + 1], src[at + 2], &Y, &cx, &cz, &yn);
      s[im][rr][0][c] = Y; s[im][rr][1][c] = cx; s[im][rr][2][c] = cz; s[im][rr][3][c] = yn;
    }
  }
  __syncthreads();
  const int rr = tid / FLIP_HW, c = tid - rr * FLIP_HW;
  const int y = y0 + rr;
  if (y >= H || c >= ncol) return;
  float acc[2][7];
#pragma unroll
  for (int im = 0; im < 2; ++im)
#pragma unroll
    for (int j = 0; j < 7; ++j) acc[im][j] = 0.f;
  for (int k = 0; k <= 2 * rs; ++k) {
    const float wa = filt.a[k], wrg = filt.rg[k], w1 = filt.b1[k], w2 = filt.b2[k];
#pragma unroll
    for (int im = 0; im < 2; ++im) {
      const float cz = s[im][rr][2][c + k];
      acc[im][0] = fmaf(wa, s[im][rr][0][c + k], acc[im][0]);
      acc[im][1] = fmaf(wrg, s[im][rr][1][c + k], acc[im][1]);
      acc[im][2] = fmaf(w1, cz, acc[im][2]);
      acc[im][3] = fmaf(w2, cz, acc[im][3]);
    }
  }
  const int off = rs - rf;
  for (int k = 0; k <= 2 * rf; ++k) {
    const float wg = filt.g[k], we = filt.e[k], wp = filt.p[k];
#pragma unroll
    for (int im = 0; im < 2; ++im) {
      const float yn = s[im][rr][3][c + off + k];
      acc[im][4] = fmaf(wg, yn, acc[im][4]);
      acc[im][5] = fmaf(we, yn, acc[im][5]);
      acc[im][6] = fmaf(wp, yn, acc[im][6]);
    }
  }
  const long long px = (img * H + y) * W + x0 + c;
#pragma unroll
  for (int im = 0; im < 2; ++im)
#pragma unroll
    for (int j = 0; j < 7; ++j) planes[(im * 7 + j) * plane_stride + px] = acc[im][j];
}

__global__ __launch_bounds__(FLIP_THREADS) void flip_vertical_kernel(const float* __restrict__ planes, long long plane_stride, int H, int W, int rs,
                                                                     int rf, int tiles_x, int tiles_y, FlipFilter filt, float cmax,
                                                                     float* __restrict__ map, double* __restrict__ partials) {
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long blk = blockIdx.x;
  const int tx = (int)(blk % tiles_x), ty = (int)((blk / tiles_x) % tiles_y);
  const long long img = blk / ((long long)tiles_x * tiles_y);
  const int x = tx * FLIP_TW + lane;
  const int i0 = ty * FLIP_TH + wave * FLIP_RPT;
  const int off = rs - rf;
  double part = 0.0;
  if (x < W && i0 < H) {
    // [row][image][A, RG, BY, edge x, edge y, point x, point y]
    float acc[FLIP_RPT][2][7];
#pragma unroll
    for (int q = 0; q < FLIP_RPT; ++q)
#pragma unroll
      for (int im = 0; im < 2; ++im)
#pragma unroll
        for (int j = 0; j < 7; ++j) acc[q][im][j] = 0.f;
    for (int r = 0; r < FLIP_RPT + 2 * rs; ++r) {
      int row = i0 + r - rs;
      row = row < 0 ? 0 : (row > H - 1 ? H - 1 : row);
      const long long px = (img * H + row) * W + x;
      float v[2][7];
#pragma unroll
      for (int im = 0; im < 2; ++im)
#pragma unroll
        for (int j = 0; j < 7; ++j) v[im][j] = planes[(im * 7 + j) * plane_stride + px];
#pragma unroll
      for (int q = 0; q < FLIP_RPT; ++q) {
        const int k = r - q;
        if (k < 0 || k > 2 * rs) continue;
        const float wa = filt.a[k], wrg = filt.rg[k], w1 = filt.vb1[k], w2 = filt.vb2[k];
#pragma unroll
        for (int im = 0; im < 2; ++im) {
          acc[q][im][0] = fmaf(wa, v[im][0], acc[q][im][0]);
          acc[q][im][1] = fmaf(wrg, v[im][1], acc[q][im][1]);
          acc[q][im][2] = fmaf(w1, v[im][2], acc[q][im][2]);
          acc[q][im][2] = fmaf(w2, v[im][3], acc[q][im][2]);
        }
        const int kf = k - off;
        if (kf < 0 || kf > 2 * rf) continue;
        const float wg = filt.g[kf], we = filt.e[kf], wp = filt.p[kf];
#pragma unroll
        for (int im = 0; im < 2; ++im) {
          acc[q][im][3] = fmaf(wg, v[im][5], acc[q][im][3]);      // the edge vector ran along x, g runs along y
          acc[q][im][4] = fmaf(we, v[im][4], acc[q][im][4]);
          acc[q][im][5] = fmaf(wg, v[im][6], acc[q][im][5]);
          acc[q][im][6] = fmaf(wp, v[im][4], acc[q][im][6]);
        }
      }
    }
    const float pccmax = 0.4f * cmax;
#pragma unroll
    for (int q = 0; q < FLIP_RPT; ++q) {
      const int i = i0 + q;
      if (i >= H) break;
      float L[2], A[2], B[2], ne[2], np[2];
#pragma unroll
      for (int im = 0; im < 2; ++im) {
        flip_hunt_lab(acc[q][im][0], acc[q][im][1], acc[q][im][2], &L[im], &A[im], &B[im]);
        ne[im] = sqrtf(acc[q][im][3] * acc[q][im][3] + acc[q][im][4] * acc[q][im][4]);
        np[im] = sqrtf(acc[q][im][5] * acc[q][im][5] + acc[q][im][6] * acc[q][im][6]);
      }
      const float dA = A[0] - A[1], dB = B[0] - B[1];
      const float hyab = fabsf(L[0] - L[1]) + sqrtf(dA * dA + dB * dB);
      const float pw = powf(hyab, 0.7f);
      const float de_c = pw < pccmax ? (0.95f / pccmax) * pw : 0.95f + ((pw - pccmax) / (cmax - pccmax)) * (1.0f - 0.95f);
      const float df = nan_max(fabsf(ne[0] - ne[1]), fabsf(np[1] - np[0]));
      const float de_f = sqrtf(0.70710678118654752f * df);
      const float m = powf(de_c, 1.f - de_f);
      if (map) map[(img * H + i) * W + x] = m;
      part += (double)m;
    }
  }
  if (partials) {
    part = block_sum4(part, red);
    if (tid == 0) partials[blk] = part;
  }
}

int flip_check(int64_t n, int32_t H, int32_t W, double ppd, FlipPlan* p) {
  RNERF_CHECK_ARG(n >= 1 && H >= 1 && W >= 1, "rnerf_flip: need n >= 1, H >= 1 and W >= 1");
  RNERF_CHECK_ARG(isfinite(ppd) && ppd > 0.0, "rnerf_flip: pixels_per_degree must be finite and > 0");
  // generate_spatial_filter (flip_api.py:313-315) and feature_detection (:411-415), in the reference's order of operations
  const double rs = ceil(3.0 * sqrt(0.04 / (2.0 * (M_PI * M_PI))) * ppd);
  const double rf = ceil(3.0 * (0.5 * 0.082 * ppd));
  if (rs > FLIP_MAX_R || rf > FLIP_MAX_R) {
    set_error("rnerf_flip: pixels_per_degree %g needs filter radii %.0f and %.0f; at most %d is supported", ppd, rs, rf, FLIP_MAX_R);
    return RNERF_ERR_UNSUPPORTED;
  }
  p->rs = (int)rs; p->rf = (int)rf;
  p->segs = (W + FLIP_HW - 1) / FLIP_HW; p->rowblks = (H + FLIP_HROWS - 1) / FLIP_HROWS;
  p->tiles_x = (W + FLIP_TW - 1) / FLIP_TW; p->tiles_y = (H + FLIP_TH - 1) / FLIP_TH;
  RNERF_CHECK_ARG((long long)n * H * W <= (1LL << 31) / 3, "rnerf_flip: n * H * W too large");
  return RNERF_OK;
}

// The 1-D vectors of the metric's filters at this pixels_per_degree, in double, rounded to float once.  false where a sum that
// normalises is 0 or not finite (a pixels_per_degree so small that every off-centre weight underflows).
bool flip_filters(double ppd, int rs, int rf, FlipFilter* f) {
  // spatial CSFs, generate_spatial_filter (flip_api.py:275-324): s = a1 sqrt(pi/b1) exp(-pi^2 z / b1) + a2 sqrt(pi/b2) exp(-pi^2 z / b2)
  // normalised by its 2-D sum, z = (x^2 + y^2) / ppd^2 rounded to float32 there; per axis z is the rounded (x / ppd)^2
  const double dx = 1.0 / ppd, pi2 = M_PI * M_PI;
  const double b_a = 0.0047, b_rg = 0.0053, a1 = 34.1, b1 = 0.04, a2 = 13.5, b2 = 0.025;
  double ga[FLIP_TAPS], grg[FLIP_TAPS], g1[FLIP_TAPS], g2[FLIP_TAPS], sa = 0, srg = 0, s1 = 0, s2 = 0;
  for (int k = 0; k <= 2 * rs; ++k) {
    const double t = (k - rs) * dx;
    const double z = (double)(float)(t * t);
    ga[k] = exp(-pi2 * z / b_a); grg[k] = exp(-pi2 * z / b_rg); g1[k] = exp(-pi2 * z / b1); g2[k] = exp(-pi2 * z / b2);
    sa += ga[k]; srg += grg[k]; s1 += g1[k]; s2 += g2[k];
  }
  const double c1 = a1 * sqrt(M_PI / b1) * s1 * s1, c2 = a2 * sqrt(M_PI / b2) * s2 * s2;     // each Gaussian's share of the 2-D sum
  if (!(sa > 0 && srg > 0 && s1 > 0 && s2 > 0 && isfinite(c1 + c2))) return false;
  for (int k = 0; k <= 2 * rs; ++k) {
    f->a[k] = (float)(ga[k] / sa); f->rg[k] = (float)(grg[k] / srg);
    f->b1[k] = (float)(g1[k] / s1); f->b2[k] = (float)(g2[k] / s2);
    f->vb1[k] = (float)(c1 / (c1 + c2) * (g1[k] / s1)); f->vb2[k] = (float)(c2 / (c1 + c2) * (g2[k] / s2));
  }
  // feature_detection (flip_api.py:400-437): g = exp(-(x^2 + y^2) / (2 sd^2)); edge -x g, point (x^2 / sd^2 - 1) g; the positive weights
  // are normalised to sum to 1 and the negative ones to -1.  The sign depends on x only, so both sums factor through sum(g(y)).
  const double sd = 0.5 * 0.082 * ppd;
  double g[FLIP_TAPS], e[FLIP_TAPS], p[FLIP_TAPS], sg = 0, epos = 0, eneg = 0, ppos = 0, pneg = 0;
  for (int k = 0; k <= 2 * rf; ++k) {
    const double x = k - rf;
    g[k] = exp(-(x * x) / (2.0 * sd * sd));
    e[k] = -x * g[k];
    p[k] = (x * x / (sd * sd) - 1.0) * g[k];
    sg += g[k];
    if (e[k] > 0) epos += e[k]; else eneg -= e[k];
    if (p[k] > 0) ppos += p[k]; else pneg -= p[k];
  }
  if (!(sg > 0 && epos > 0 && eneg > 0 && ppos > 0 && pneg > 0 && isfinite(sg))) return false;
  for (int k = 0; k <= 2 * rf; ++k) {
    f->g[k] = (float)(g[k] / sg);
    f->e[k] = (float)(e[k] < 0 ? e[k] / eneg : e[k] / epos);
    f->p[k] = (float)(p[k] < 0 ? p[k] / pneg : p[k] / ppos);
  }
  return true;
}

// cmax (flip_api.py:473-475): the HyAB distance of Hunt-adjusted green and blue, ^0.7.  A constant of the metric.
float flip_cmax() {
  auto lab_f = [](double t) { const double d = 6.0 / 29.0; return t > d * d * d ? cbrt(t) : t / (3.0 * d * d) + 4.0 / 29.0; };
  auto hunt_lab = [&](double x, double y, double z, double* o) {
    const double fx = lab_f(x * (double)FLIP_IWX), fy = lab_f(y), fz = lab_f(z * (double)FLIP_IWZ);
    o[0] = 116.0 * fy - 16.0;
    o[1] = 0.01 * o[0] * (500.0 * (fx - fy));
    o[2] = 0.01 * o[0] * (200.0 * (fy - fz));
  };
  double gr[3], bl[3];
  hunt_lab(FLIP_A12, FLIP_A22, FLIP_A32, gr);
  hunt_lab(FLIP_A13, FLIP_A23, FLIP_A33, bl);
  const double da = gr[1] - bl[1], db = gr[2] - bl[2];
  return (float)pow(fabs(gr[0] - bl[0]) + sqrt(da * da + db * db), 0.7);
}

inline size_t flip_partials_bytes(int64_t n, const FlipPlan& p) { return (size_t)n * p.tiles_x * p.tiles_y * sizeof(double); }

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
  SsimFilter filt;
  const double sum = ssim_taps(fs, [&](int i) { const double t = (i - hw + shift) / filter_sigma; return -0.5 * t * t; }, &filt);
  RNERF_CHECK_ARG(sum > 0.0 && isfinite(sum), "rnerf_ssim: the filter's weights sum to %g", sum);
  const float c1 = (float)((k1 * max_val) * (k1 * max_val)), c2 = (float)((k2 * max_val) * (k2 * max_val));
  const long long tiles = (long long)p.tiles_x * p.tiles_y;
  hipStream_t st = (hipStream_t)stream;
  double* partials = mean ? (double*)workspace : nullptr;
  const int launched = ssim_launch<false>(p, filt, c1, c2, img0, img1, n, H, W, C, fs, map, partials, st);
  if (launched != RNERF_OK) return launched;
  if (mean) {
    const double count = (double)(H - fs + 1) * (double)(W - fs + 1) * (double)C;
    hipLaunchKernelGGL(ssim_mean_kernel, dim3((unsigned)n), dim3(SSIM_THREADS), 0, st, partials, (int)tiles, count, mean);
    RNERF_CHECK_LAUNCH();
  }
  return RNERF_OK;
}

extern "C" size_t rnerf_errmap_mse_workspace_bytes(int64_t n, int32_t H, int32_t W) {
  long long bpi;
  if (errmap_mse_check(n, H, W, 1, &bpi) != RNERF_OK) return 0;
  return (size_t)n * (size_t)bpi * sizeof(double);
}

extern "C" int rnerf_errmap_mse(const float* reference, const float* test, int64_t n, int32_t H, int32_t W, int32_t C, float* map, float* mean,
                                void* workspace, void* stream) {
  long long bpi;
  const int rc = errmap_mse_check(n, H, W, C, &bpi);
  if (rc != RNERF_OK) return rc;
  RNERF_CHECK_ARG(reference && test && (map || mean), "rnerf_errmap_mse: null pointer (reference, test, and map or mean)");
  RNERF_CHECK_ARG(!mean || workspace, "rnerf_errmap_mse: the mean needs the workspace (rnerf_errmap_mse_workspace_bytes)");
  RNERF_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "rnerf_errmap_mse: the workspace must be 8-byte aligned");
  const long long hw = (long long)H * W;
  const size_t in_bytes = (size_t)n * hw * C * sizeof(float);
  if (map)
    RNERF_CHECK_ARG(!overlaps(map, (size_t)n * hw * sizeof(float), reference, in_bytes) && !overlaps(map, (size_t)n * hw * sizeof(float), test, in_bytes),
                    "rnerf_errmap_mse: map overlaps an input");
  hipStream_t st = (hipStream_t)stream;
  double* partials = mean ? (double*)workspace : nullptr;
  hipLaunchKernelGGL(errmap_mse_kernel, dim3((unsigned)(n * bpi)), dim3(SSIM_THREADS), 0, st, reference, test, hw, C, (int)bpi, map, partials);
  RNERF_CHECK_LAUNCH();
  if (mean) {
    hipLaunchKernelGGL(ssim_mean_kernel, dim3((unsigned)n), dim3(SSIM_THREADS), 0, st, partials, (int)bpi, (double)hw * (double)C, mean);
    RNERF_CHECK_LAUNCH();
  }
  return RNERF_OK;
}

// workspace of rnerf_ssim_summary: one fp64 partial per tile, then the per-channel map float[n][H-fs+1][W-fs+1][C]
inline size_t ssim_summary_partials_bytes(int64_t n, const SsimPlan& p) { return (size_t)n * p.tiles_x * p.tiles_y * sizeof(double); }

extern "C" size_t rnerf_ssim_summary_workspace_bytes(int64_t n, int32_t H, int32_t W, int32_t C, int32_t filter_size) {
  SsimPlan p;
  if (ssim_check(n, H, W, C, filter_size, &p) != RNERF_OK) return 0;
  return ssim_summary_partials_bytes(n, p) + (size_t)n * (H - filter_size + 1) * (W - filter_size + 1) * C * sizeof(float);
}

extern "C" int rnerf_ssim_summary(const float* img0, const float* img1, int64_t n, int32_t H, int32_t W, int32_t C, int32_t filter_size,
                                  double filter_sigma, double data_range, float* map, float* mean, void* workspace, void* stream) {
  SsimPlan p;
  const int rc = ssim_check(n, H, W, C, filter_size, &p);
  if (rc != RNERF_OK) return rc;
  RNERF_CHECK_ARG(filter_sigma > 0.0 && isfinite(filter_sigma), "rnerf_ssim_summary: filter_sigma must be finite and > 0");
  RNERF_CHECK_ARG(isfinite(data_range), "rnerf_ssim_summary: data_range must be finite");
  RNERF_CHECK_ARG(img0 && img1 && (map || mean), "rnerf_ssim_summary: null pointer (img0, img1, and map or mean)");
  RNERF_CHECK_ARG(workspace, "rnerf_ssim_summary: the per-channel map and the mean need the workspace (rnerf_ssim_summary_workspace_bytes)");
  RNERF_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "rnerf_ssim_summary: the workspace must be 8-byte aligned");
  // _fspecial_gauss_1d (ssim.py:20-24), in double, rounded once
  const int fs = filter_size;
  SsimFilter filt;
  const double sum = ssim_taps(fs, [&](int i) { const double t = (double)(i - fs / 2); return -(t * t) / (2.0 * filter_sigma * filter_sigma); }, &filt);
  RNERF_CHECK_ARG(sum > 0.0 && isfinite(sum), "rnerf_ssim_summary: the filter's weights sum to %g", sum);
  const float c1 = (float)((0.01 * data_range) * (0.01 * data_range)), c2 = (float)((0.03 * data_range) * (0.03 * data_range));
  const long long tiles = (long long)p.tiles_x * p.tiles_y;
  hipStream_t st = (hipStream_t)stream;
  double* partials = mean ? (double*)workspace : nullptr;
  float* per_channel = map ? (float*)((char*)workspace + ssim_summary_partials_bytes(n, p)) : nullptr;
  const int launched = ssim_launch<true>(p, filt, c1, c2, img0, img1, n, H, W, C, fs, per_channel, partials, st);
  if (launched != RNERF_OK) return launched;
  const long long pixels = n * (long long)(H - fs + 1) * (W - fs + 1);
  if (map) {
    hipLaunchKernelGGL(channel_mean_kernel, dim3((unsigned)((pixels + SSIM_THREADS - 1) / SSIM_THREADS)), dim3(SSIM_THREADS), 0, st, per_channel, pixels, C, map);
    RNERF_CHECK_LAUNCH();
  }
  if (mean) {
    hipLaunchKernelGGL(ssim_mean_kernel, dim3((unsigned)n), dim3(SSIM_THREADS), 0, st, partials, (int)tiles, (double)pixels / (double)n * (double)C, mean);
    RNERF_CHECK_LAUNCH();
  }
  return RNERF_OK;
}

extern "C" size_t rnerf_flip_workspace_bytes(int64_t n, int32_t H, int32_t W, double pixels_per_degree) {
  FlipPlan p;
  FlipFilter filt;
  if (flip_check(n, H, W, pixels_per_degree, &p) != RNERF_OK) return 0;
  if (!flip_filters(pixels_per_degree, p.rs, p.rf, &filt)) {
    set_error("rnerf_flip: the filter weights at pixels_per_degree %g do not sum to a positive finite value", pixels_per_degree);
    return 0;
  }
  return flip_partials_bytes(n, p) + (size_t)FLIP_PLANES * n * H * W * sizeof(float);
}

extern "C" int rnerf_flip(const float* reference, const float* test, int64_t n, int32_t H, int32_t W, double pixels_per_degree, float* map,
                          float* mean, void* workspace, void* stream) {
  FlipPlan p;
  const int rc = flip_check(n, H, W, pixels_per_degree, &p);
  if (rc != RNERF_OK) return rc;
  RNERF_CHECK_ARG(reference && test && (map || mean), "rnerf_flip: null pointer (reference, test, and map or mean)");
  RNERF_CHECK_ARG(workspace, "rnerf_flip: the filtered planes and the mean need the workspace (rnerf_flip_workspace_bytes)");
  RNERF_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "rnerf_flip: the workspace must be 8-byte aligned");
  FlipFilter filt = {};
  if (!flip_filters(pixels_per_degree, p.rs, p.rf, &filt)) {
    set_error("rnerf_flip: the filter weights at pixels_per_degree %g do not sum to a positive finite value", pixels_per_degree);
    return RNERF_ERR_UNSUPPORTED;
  }
  const float cmax = flip_cmax();
  hipStream_t st = (hipStream_t)stream;
  double* partials = (double*)workspace;                                  // one per vertical-pass tile, then the 14 planes
  float* planes = (float*)((char*)workspace + flip_partials_bytes(n, p));
  const long long plane_stride = (long long)n * H * W;
  hipLaunchKernelGGL(flip_horizontal_kernel, dim3((unsigned)(n * p.segs * p.rowblks)), dim3(FLIP_THREADS), 0, st, reference, test, H, W, p.rs, p.rf,
                     p.segs, p.rowblks, filt, planes, plane_stride);
  RNERF_CHECK_LAUNCH();
  const long long tiles = (long long)p.tiles_x * p.tiles_y;
  hipLaunchKernelGGL(flip_vertical_kernel, dim3((unsigned)(n * tiles)), dim3(FLIP_THREADS), 0, st, planes, plane_stride, H, W, p.rs, p.rf, p.tiles_x,
                     p.tiles_y, filt, cmax, map, mean ? partials : nullptr);
  RNERF_CHECK_LAUNCH();
  if (mean) {
    hipLaunchKernelGGL(ssim_mean_kernel, dim3((unsigned)n), dim3(SSIM_THREADS), 0, st, partials, (int)tiles, (double)H * (double)W, mean);
    RNERF_CHECK_LAUNCH();
  }
  return RNERF_OK;
}
