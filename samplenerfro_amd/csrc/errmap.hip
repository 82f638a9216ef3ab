// The comparison sheet of metric/summary.py on the device: ground truth | prediction | the coloured error maps side by side as finished
// bytes (summary.py:40-45, :223-240), so that one uint8 image per view crosses the bus.  The maps themselves are made in metrics.hip:
// the squared error (rnerf_errmap_mse), the summary SSIM (rnerf_ssim_summary) and FLIP (rnerf_flip).
//
// One streaming kernel: no LDS beyond the 768-byte colour table, no atomics.
//
// Below it, the A/B comparison of two runs (metric/compare.py:216-236, metric/export.py:92-133): the win/loss frame with its integer
// counts (rnerf_compare_sheet) and the side-by-side strip (rnerf_compare_strip), two more streaming kernels of the same byte ownership.
#include "common.h"
#include "eval_host.h"
#include "magma_table.h"

namespace rnerf {
namespace {

constexpr int ERRMAP_THREADS = 256;
constexpr int SHEET_MAX_MAPS = 4;
constexpr int SHEET_GAP = 5;                 // summary.py:231,238: np.ones((h, 5, 3)) between the panels and after the last

__device__ const unsigned char magma_lut[768] = RNERF_MAGMA_TABLE;

struct SheetMaps {
  const float* p[SHEET_MAX_MAPS];
  int h[SHEET_MAX_MAPS], w[SHEET_MAX_MAPS];
};

// save_img (summary.py:40-41) on the float64 hstack: trunc(clip(255.0 * double(x), 0, 255)).  NaN (and anything below 0) gives 0.
__device__ __forceinline__ unsigned sheet_image_byte(float x) {
  const double v = 255.0 * (double)x;
  if (!(v >= 0.0)) return 0u;
  return (unsigned)(v > 255.0 ? 255.0 : v);
}

// save_err's index (summary.py:44, index2color's astype(int)): trunc(clip(255.0 * v, 0, 255)), the product in float32.  NaN gives 0.
__device__ __forceinline__ unsigned sheet_map_index(float m) {
  const float v = fmul(255.0f, m);
  if (!(v >= 0.0f)) return 0u;
  return (unsigned)(v > 255.0f ? 255.0f : v);
}

// One byte of the sheet.  xb: byte offset within the row, row_px = (2 + K) (W + 5) pixels wide.
__device__ __forceinline__ unsigned sheet_byte(const float* __restrict__ ref, const float* __restrict__ test, const SheetMaps& maps, int W,
                                               int y, int xb, const unsigned char* lut) {
  const int col = xb / 3, c = xb - 3 * col;
  const int panel = col / (W + SHEET_GAP), x = col - panel * (W + SHEET_GAP);
  if (x >= W) return 255u;
  if (panel < 2) {
    const float* __restrict__ src = panel == 0 ? ref : test;
    return sheet_image_byte(src[((long long)y * W + x) * 3 + c]);
  }
  const int k = panel - 2;
  if (y >= maps.h[k] || x >= maps.w[k]) return 0u;
  return lut[3 * sheet_map_index(maps.p[k][(long long)y * maps.w[k] + x]) + c];
}

// A thread owns 4 consecutive bytes of the flat output (rows are (2 + K) (W + 5) 3 bytes, not a multiple of 4 in general, so a thread's
// bytes may span two rows) and writes them with one 32-bit store; a wave writes 256 consecutive bytes.  The last thread writes what is
// left byte by byte, and so does every thread when `out` is not 4-byte aligned.
__global__ __launch_bounds__(ERRMAP_THREADS) void errmap_sheet_kernel(const float* __restrict__ ref, const float* __restrict__ test, SheetMaps maps,
                                                                      int W, int row_bytes, long long total, int vec,
                                                                      unsigned char* __restrict__ out) {
  __shared__ unsigned char lut[768];
  for (int i = threadIdx.x; i < 768; i += ERRMAP_THREADS) lut[i] = magma_lut[i];
  __syncthreads();
  const long long at = ((long long)blockIdx.x * ERRMAP_THREADS + threadIdx.x) * 4;
  if (at >= total) return;
  int y = (int)(at / row_bytes), xb = (int)(at - (long long)y * row_bytes);
  const int n = total - at < 4 ? (int)(total - at) : 4;
  unsigned b[4] = {0u, 0u, 0u, 0u};
  for (int e = 0; e < n; ++e) {
    b[e] = sheet_byte(ref, test, maps, W, y, xb, lut);
    if (++xb == row_bytes) { xb = 0; ++y; }
  }
  if (vec && n == 4) {
    *reinterpret_cast<uint32_t*>(out + at) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
  } else {
    for (int e = 0; e < n; ++e) out[at + e] = (unsigned char)b[e];
  }
}

// ---- metric/compare.py:216-236: which of two runs has the lower error, per pixel and metric ------------------------------------------

constexpr int CMP_A = 0, CMP_TIE = 1, CMP_B = 2, CMP_NEITHER = 3;

struct CompareMaps {
  const float* a[SHEET_MAX_MAPS];
  const float* b[SHEET_MAX_MAPS];
  int h[SHEET_MAX_MAPS], w[SHEET_MAX_MAPS];
};

// compare.py:221-223.  non = |a - b| < 1e-3 (one rounded float32 subtraction; no float32 lies between 1e-3 and float32(1e-3)),
// pos = !non && a <= b, neg = !non && a > b.  A NaN on either side fails all three; inf - inf is NaN, so equal infinities are "A wins".
__device__ __forceinline__ int compare_class(float a, float b) {
  const float d = fabsf(fsub(a, b));
  if (d < 1e-3f) return CMP_TIE;
  if (a <= b) return CMP_A;
  return a > b ? CMP_B : CMP_NEITHER;
}

// compare.py:225-227 through save_img (:40): trunc(clip(255.0 * (c / 255.0))) is c for these nine components (tests/test_compare_host.py).
__device__ __forceinline__ unsigned compare_colour(int cls, int c) {
  const unsigned rgb = cls == CMP_A ? 0x628AEFu : cls == CMP_TIE ? 0xF7F7F7u : cls == CMP_B ? 0xCFA967u : 0u;      // byte c of (239, 138, 98) ...
  return (rgb >> (8 * c)) & 255u;
}

constexpr int COMPARE_MAX_BLOCKS = 2048;     // 8 workgroups a CU; the rest of the frame is walked in a grid-stride loop

// The byte ownership of errmap_sheet_kernel, 4 consecutive bytes of the flat output per thread and step, in a grid-stride loop over
// steps of 1024 bytes: every workgroup adds to `counts` once, at its end — with one workgroup per 1024 bytes the 16 counters, not the
// memory, set the pace (7547 workgroups at 800 x 800 and K = 4).  A row is K (W + 5) 3 bytes; a gap is 15 bytes, so the 4 bytes touch
// one panel at most and hold at most two first-channel bytes.  A thread keeps the counts of panel k as four fields of 16 bits in
// acc[k]: a frame below 2^31 bytes is at most 2^21 steps, 1024 a thread over COMPARE_MAX_BLOCKS workgroups, so a field is at most
// 2048.  At the end each field is summed over the wave by shuffles, over the workgroup in LDS, and added to `counts` with one integer
// atomic per non-zero counter.  Integer sums: the same on every run.
__global__ __launch_bounds__(ERRMAP_THREADS) void compare_sheet_kernel(CompareMaps maps, int K, int W, int row_bytes, long long total, int vec,
                                                                       unsigned char* __restrict__ out, unsigned long long* __restrict__ counts) {
  __shared__ unsigned block_counts[SHEET_MAX_MAPS * 4];
  if (counts) {
    if (threadIdx.x < SHEET_MAX_MAPS * 4) block_counts[threadIdx.x] = 0u;
    __syncthreads();
  }
  unsigned long long acc[SHEET_MAX_MAPS] = {0ull, 0ull, 0ull, 0ull};
  const long long stride = (long long)gridDim.x * ERRMAP_THREADS * 4;
  for (long long at = ((long long)blockIdx.x * ERRMAP_THREADS + threadIdx.x) * 4; at < total; at += stride) {
    const int n = total - at < 4 ? (int)(total - at) : 4;
    int y = (int)((unsigned)at / (unsigned)row_bytes), xb = (int)((unsigned)at - (unsigned)y * (unsigned)row_bytes);      // at < total < 2^31
    int col = xb / 3, c = xb - 3 * col;
    int cls = -1;                                 // the class of pixel `col`, once it is known
    unsigned b[4] = {0u, 0u, 0u, 0u};
    unsigned long long mine = 0ull;
    int panel = 0;
    for (int e = 0; e < n; ++e) {
      const int p = col / (W + SHEET_GAP), x = col - p * (W + SHEET_GAP);
      if (x >= W || y >= maps.h[p] || x >= maps.w[p]) {
        b[e] = 255u;                              // compare.py:230,234: np.ones
      } else {
        if (cls < 0) {
          const long long i = (long long)y * maps.w[p] + x;
          cls = compare_class(maps.a[p][i], maps.b[p][i]);
        }
        if (c == 0) { mine += 1ull << (16 * cls); panel = p; }
        b[e] = compare_colour(cls, c);
      }
      ++xb;
      if (++c == 3) { c = 0; ++col; cls = -1; }
      if (xb == row_bytes) { xb = 0; col = 0; ++y; }
    }
    if (vec && n == 4) {
      *reinterpret_cast<uint32_t*>(out + at) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    } else {
      for (int e = 0; e < n; ++e) out[at + e] = (unsigned char)b[e];
    }
#pragma unroll
    for (int k = 0; k < SHEET_MAX_MAPS; ++k) acc[k] += panel == k ? mine : 0ull;       // no dynamic index: acc stays in registers
  }
  if (!counts) return;
#pragma unroll
  for (int k = 0; k < SHEET_MAX_MAPS; ++k) {
    if (k >= K) break;
#pragma unroll
    for (int cls = 0; cls < 4; ++cls) {
      unsigned v = (unsigned)(acc[k] >> (16 * cls)) & 0xFFFFu;
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if ((threadIdx.x & 63) == 0 && v) atomicAdd(&block_counts[4 * k + cls], v);
    }
  }
  __syncthreads();
  if (threadIdx.x < 4 * K && block_counts[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)block_counts[threadIdx.x]);
}

// ---- metric/export.py:92-133: the runs and the ground truth side by side -------------------------------------------------------------

struct StripImages {
  const unsigned char* p[SHEET_MAX_MAPS];
};

struct StripTable {
  unsigned char v[256];                           // export.py:105 at weight 0.5 for every byte, made on the host in double
};

__global__ __launch_bounds__(ERRMAP_THREADS) void compare_strip_kernel(StripImages images, int N, const unsigned char* __restrict__ reference,
                                                                       StripTable table, int W, int rx0, int ry0, int rx1, int ry1, int fade,
                                                                       int row_bytes, long long total, int vec, unsigned char* __restrict__ out) {
  __shared__ unsigned char lut[256];
  lut[threadIdx.x] = table.v[threadIdx.x];        // ERRMAP_THREADS == 256
  __syncthreads();
  const long long at = ((long long)blockIdx.x * ERRMAP_THREADS + threadIdx.x) * 4;
  if (at >= total) return;
  int y = (int)((unsigned)at / (unsigned)row_bytes), xb = (int)((unsigned)at - (unsigned)y * (unsigned)row_bytes);        // at < total < 2^31
  const int n = total - at < 4 ? (int)(total - at) : 4;
  const int ref_at = N * (W + SHEET_GAP);         // the reference's first column
  unsigned b[4] = {0u, 0u, 0u, 0u};
  for (int e = 0; e < n; ++e) {
    const int col = xb / 3, c = xb - 3 * col;
    if (col >= ref_at) {
      b[e] = reference[((long long)y * W + (col - ref_at)) * 3 + c];                  // export.py fades only the predictions
    } else {
      const int p = col / (W + SHEET_GAP), x = col - p * (W + SHEET_GAP);
      if (x >= W) {
        b[e] = 255u;
      } else {
        const unsigned v = images.p[p][((long long)y * W + x) * 3 + c];
        const bool inside = x >= rx0 && x < rx1 && y >= ry0 && y < ry1;
        b[e] = fade && !inside ? lut[v] : v;
      }
    }
    if (++xb == row_bytes) { xb = 0; ++y; }
  }
  if (vec && n == 4) {
    *reinterpret_cast<uint32_t*>(out + at) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
  } else {
    for (int e = 0; e < n; ++e) out[at + e] = (unsigned char)b[e];
  }
}

}  // namespace
}  // namespace rnerf

using namespace rnerf;

extern "C" int rnerf_errmap_sheet(const float* reference, const float* test, int32_t H, int32_t W, int32_t K, const float* const* maps,
                                  const int32_t* map_h, const int32_t* map_w, uint8_t* out, void* stream) {
  RNERF_CHECK_ARG(reference && test && out, "rnerf_errmap_sheet: null pointer (reference, test or out)");
  RNERF_CHECK_ARG(K >= 0 && K <= SHEET_MAX_MAPS, "rnerf_errmap_sheet: K must be in [0, %d], got %d", SHEET_MAX_MAPS, K);
  RNERF_CHECK_ARG(K == 0 || (maps && map_h && map_w), "rnerf_errmap_sheet: null pointer (maps, map_h or map_w)");
  RNERF_CHECK_ARG(H >= 1 && W >= 1, "rnerf_errmap_sheet: need H >= 1 and W >= 1");
  const long long row_bytes = (long long)(2 + K) * ((long long)W + SHEET_GAP) * 3;
  const long long total = row_bytes * H;
  RNERF_CHECK_ARG(total < (1LL << 31), "rnerf_errmap_sheet: the sheet must be below 2^31 bytes");
  const size_t in_bytes = (size_t)H * W * 3 * sizeof(float);
  RNERF_CHECK_ARG(!overlaps(out, (size_t)total, reference, in_bytes) && !overlaps(out, (size_t)total, test, in_bytes),
                  "rnerf_errmap_sheet: out overlaps an input image");
  SheetMaps m = {};
  for (int k = 0; k < K; ++k) {
    RNERF_CHECK_ARG(maps[k], "rnerf_errmap_sheet: null pointer (map %d)", k);
    RNERF_CHECK_ARG(map_h[k] >= 1 && map_w[k] >= 1 && map_h[k] <= H && map_w[k] <= W,
                    "rnerf_errmap_sheet: map %d is %d x %d, it must be non-empty and no larger than the image (%d x %d)", k, map_h[k], map_w[k], H, W);
    RNERF_CHECK_ARG(!overlaps(out, (size_t)total, maps[k], (size_t)map_h[k] * map_w[k] * sizeof(float)), "rnerf_errmap_sheet: out overlaps map %d", k);
    m.p[k] = maps[k]; m.h[k] = map_h[k]; m.w[k] = map_w[k];
  }
  const long long threads = (total + 3) / 4;
  const int vec = ((uintptr_t)out & 3) == 0;
  hipLaunchKernelGGL(errmap_sheet_kernel, dim3((unsigned)((threads + ERRMAP_THREADS - 1) / ERRMAP_THREADS)), dim3(ERRMAP_THREADS), 0, (hipStream_t)stream,
                     reference, test, m, W, (int)row_bytes, total, vec, out);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_compare_sheet(int32_t H, int32_t W, int32_t K, const float* const* maps_a, const float* const* maps_b, const int32_t* map_h,
                                   const int32_t* map_w, uint8_t* out, int64_t* counts, void* stream) {
  RNERF_CHECK_ARG(maps_a && maps_b && map_h && map_w && out, "rnerf_compare_sheet: null pointer (maps_a, maps_b, map_h, map_w or out)");
  RNERF_CHECK_ARG(K >= 1 && K <= SHEET_MAX_MAPS, "rnerf_compare_sheet: K must be in [1, %d], got %d", SHEET_MAX_MAPS, K);
  RNERF_CHECK_ARG(H >= 1 && W >= 1, "rnerf_compare_sheet: need H >= 1 and W >= 1");
  const long long row_bytes = (long long)K * ((long long)W + SHEET_GAP) * 3;
  const long long total = row_bytes * H;
  RNERF_CHECK_ARG(total < (1LL << 31), "rnerf_compare_sheet: the frame must be below 2^31 bytes");
  RNERF_CHECK_ARG(((uintptr_t)counts & 7) == 0, "rnerf_compare_sheet: counts must be 8-byte aligned");
  const size_t count_bytes = (size_t)K * 4 * sizeof(int64_t);
  RNERF_CHECK_ARG(!overlaps(out, (size_t)total, counts, count_bytes), "rnerf_compare_sheet: out overlaps counts");
  CompareMaps m = {};
  for (int k = 0; k < K; ++k) {
    RNERF_CHECK_ARG(maps_a[k] && maps_b[k], "rnerf_compare_sheet: null pointer (map %d)", k);
    RNERF_CHECK_ARG(map_h[k] >= 1 && map_w[k] >= 1 && map_h[k] <= H && map_w[k] <= W,
                    "rnerf_compare_sheet: map %d is %d x %d, it must be non-empty and no larger than the image (%d x %d)", k, map_h[k], map_w[k], H, W);
    const size_t map_bytes = (size_t)map_h[k] * map_w[k] * sizeof(float);
    RNERF_CHECK_ARG(!overlaps(out, (size_t)total, maps_a[k], map_bytes) && !overlaps(out, (size_t)total, maps_b[k], map_bytes),
                    "rnerf_compare_sheet: out overlaps map %d", k);
    RNERF_CHECK_ARG(!overlaps(counts, count_bytes, maps_a[k], map_bytes) && !overlaps(counts, count_bytes, maps_b[k], map_bytes),
                    "rnerf_compare_sheet: counts overlaps map %d", k);
    m.a[k] = maps_a[k]; m.b[k] = maps_b[k]; m.h[k] = map_h[k]; m.w[k] = map_w[k];
  }
  hipStream_t st = (hipStream_t)stream;
  if (counts) RNERF_CHECK_HIP(hipMemsetAsync(counts, 0, count_bytes, st));
  const long long threads = (total + 3) / 4;
  const int vec = ((uintptr_t)out & 3) == 0;
  const long long blocks = (threads + ERRMAP_THREADS - 1) / ERRMAP_THREADS;
  hipLaunchKernelGGL(compare_sheet_kernel, dim3((unsigned)(blocks < COMPARE_MAX_BLOCKS ? blocks : COMPARE_MAX_BLOCKS)), dim3(ERRMAP_THREADS), 0, st, m, K, W,
                     (int)row_bytes, total, vec, out, reinterpret_cast<unsigned long long*>(counts));
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_compare_strip(const uint8_t* const* images, int32_t N, const uint8_t* reference, int32_t H, int32_t W, int32_t rx, int32_t ry,
                                   int32_t rw, int32_t rh, uint8_t* out, void* stream) {
  RNERF_CHECK_ARG(images && reference && out, "rnerf_compare_strip: null pointer (images, reference or out)");
  RNERF_CHECK_ARG(N >= 1 && N <= SHEET_MAX_MAPS, "rnerf_compare_strip: N must be in [1, %d], got %d", SHEET_MAX_MAPS, N);
  RNERF_CHECK_ARG(H >= 1 && W >= 1, "rnerf_compare_strip: need H >= 1 and W >= 1");
  const int fade = rw != 0 && rh != 0;
  if (fade)
    RNERF_CHECK_ARG(rx >= 0 && ry >= 0 && rw >= 1 && rh >= 1 && (long long)rx + rw <= W && (long long)ry + rh <= H,
                    "rnerf_compare_strip: the rectangle (x %d, y %d, %d x %d) must lie inside the image (%d x %d)", rx, ry, rw, rh, W, H);
  const long long row_bytes = ((long long)N * ((long long)W + SHEET_GAP) + W) * 3;
  const long long total = row_bytes * H;
  RNERF_CHECK_ARG(total < (1LL << 31), "rnerf_compare_strip: the strip must be below 2^31 bytes");
  const size_t in_bytes = (size_t)H * W * 3;
  RNERF_CHECK_ARG(!overlaps(out, (size_t)total, reference, in_bytes), "rnerf_compare_strip: out overlaps the reference");
  StripImages im = {};
  for (int i = 0; i < N; ++i) {
    RNERF_CHECK_ARG(images[i], "rnerf_compare_strip: null pointer (image %d)", i);
    RNERF_CHECK_ARG(!overlaps(out, (size_t)total, images[i], in_bytes), "rnerf_compare_strip: out overlaps image %d", i);
    im.p[i] = images[i];
  }
  // export.py:103-105: np.clip(((v / 255.0) * weight + 1.0 * (1 - weight)) * 255.0, 0, 255).astype(np.uint8) at weight 0.5, in double
  StripTable table;
  for (int v = 0; v < 256; ++v) {
    const double weight = 0.5;
    double t = ((v / 255.0) * weight + 1.0 * (1.0 - weight)) * 255.0;
    t = t < 0.0 ? 0.0 : t > 255.0 ? 255.0 : t;
    table.v[v] = (unsigned char)t;
  }
  const long long threads = (total + 3) / 4;
  const int vec = ((uintptr_t)out & 3) == 0;
  hipLaunchKernelGGL(compare_strip_kernel, dim3((unsigned)((threads + ERRMAP_THREADS - 1) / ERRMAP_THREADS)), dim3(ERRMAP_THREADS), 0,
                     (hipStream_t)stream, im, N, reference, table, W, rx, ry, rx + rw, ry + rh, fade, (int)row_bytes, total, vec, out);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}
