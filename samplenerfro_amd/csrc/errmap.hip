// The comparison sheet of metric/summary.py on the device: ground truth | prediction | the coloured error maps side by side as finished
// bytes (summary.py:40-45, :223-240), so that one uint8 image per view crosses the bus.  The maps themselves are made in metrics.hip:
// the squared error (rnerf_errmap_mse), the summary SSIM (rnerf_ssim_summary) and FLIP (rnerf_flip).
//
// One streaming kernel: no LDS beyond the 768-byte colour table, no atomics.
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
