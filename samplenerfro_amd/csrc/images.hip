// Scene images: decoded 8-bit views -> the float32 [n, h, w, 3] tensor the batcher and the evaluation loop read.
// Reference: rnerf/datasets.py:348-364 (Blender), :394-414 (NSVF), :443-459 (OpenCV) — `np.array(Image.open(f), float32) / 255.`, the
// cv2.INTER_AREA halving of `factor: 2`, and the composite over white.  The reference does this on the host in float32, one image at a
// time; here the uint8 pixels are uploaded as they were decoded (a quarter of the bytes) and one streaming kernel does the three steps.
// One thread per OUTPUT pixel, 64-bit flat indices, a whole-pixel 32-bit load for RGBA and byte loads for RGB; no LDS, no atomics.
#include "common.h"

namespace rnerf {

// The channels of one source pixel as integers (RGB leaves a = 0; it is never read).
struct Px { unsigned r, g, b, a; };

template <int C>
__device__ __forceinline__ Px load_px(const uint8_t* __restrict__ src, long long pixel) {
  Px p;
  if constexpr (C == 4) {
    const uint32_t v = *(const uint32_t*)(src + pixel * 4);      // little endian: R is the low byte
    p.r = v & 255u; p.g = (v >> 8) & 255u; p.b = (v >> 16) & 255u; p.a = v >> 24;
  } else {
    const uint8_t* q = src + pixel * 3;
    p.r = q[0]; p.g = q[1]; p.b = q[2]; p.a = 0u;
  }
  return p;
}

// FACTOR 1: x = float(u) / 255.  FACTOR 2: x = float(u00 + u01 + u10 + u11) / 1020 — the mean of the 2 x 2 block from its exact integer
// sum (<= 1020), alpha included.  WHITE: x_c * x_a + (1 - x_a) on those values (datasets.py:359-362).  Every operation is one correctly
// rounded float32 operation (a true division: -fhip-fp32-correctly-rounded-divide-sqrt, and fdiv / fmul / fadd are never contracted).
template <int C, int FACTOR, bool WHITE>
__global__ void __launch_bounds__(256) images_prepare_kernel(const uint8_t* __restrict__ src, long long total, int w,
                                                             float* __restrict__ dst) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;      // output pixel, flat over (image, row, column)
  if (id >= total) return;
  Px s;
  if constexpr (FACTOR == 1) {
    s = load_px<C>(src, id);
  } else {
    const long long row = id / w;                                      // output row, flat over (image, row): source rows 2 row, 2 row + 1
    const int col = (int)(id - row * w);
    const long long W = 2LL * w, p0 = 2 * row * W + 2 * col;           // source pixel (2 row, 2 col); H is even, so images keep their parity
    const Px a = load_px<C>(src, p0), b = load_px<C>(src, p0 + 1), c = load_px<C>(src, p0 + W), d = load_px<C>(src, p0 + W + 1);
    s.r = (a.r + b.r) + (c.r + d.r); s.g = (a.g + b.g) + (c.g + d.g); s.b = (a.b + b.b) + (c.b + d.b); s.a = (a.a + b.a) + (c.a + d.a);
  }
  const float den = FACTOR == 1 ? 255.0f : 1020.0f;
  float r = fdiv((float)s.r, den), g = fdiv((float)s.g, den), b = fdiv((float)s.b, den);
  if constexpr (WHITE) {
    const float al = fdiv((float)s.a, den), bg = fsub(1.0f, al);
    r = fadd(fmul(r, al), bg); g = fadd(fmul(g, al), bg); b = fadd(fmul(b, al), bg);
  }
  float* o = dst + id * 3;
  o[0] = r; o[1] = g; o[2] = b;
}

template <int C, int FACTOR, bool WHITE>
static void launch_images_prepare(const uint8_t* src, long long total, int w, float* dst, hipStream_t stream) {
  hipLaunchKernelGGL((images_prepare_kernel<C, FACTOR, WHITE>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, src, total, w, dst);
}

}  // namespace rnerf

using namespace rnerf;

extern "C" int rnerf_images_prepare(const uint8_t* src, int64_t n, int32_t H, int32_t W, int32_t C, int32_t factor, int32_t white_bkgd,
                                    float* dst, void* stream) {
  RNERF_CHECK_ARG(src && dst, "rnerf_images_prepare: null pointer");
  RNERF_CHECK_ARG(C == 3 || C == 4, "rnerf_images_prepare: C must be 3 (RGB) or 4 (RGBA), got %d", C);
  RNERF_CHECK_ARG(factor == 1 || factor == 2, "rnerf_images_prepare: factor must be 1 or 2, got %d", factor);
  RNERF_CHECK_ARG(white_bkgd == 0 || white_bkgd == 1, "rnerf_images_prepare: white_bkgd must be 0 or 1");
  RNERF_CHECK_ARG(!(white_bkgd && C != 4), "rnerf_images_prepare: white_bkgd needs an alpha channel (C == 4)");
  RNERF_CHECK_ARG(n >= 1 && H >= 1 && W >= 1, "rnerf_images_prepare: need n, H, W >= 1");
  RNERF_CHECK_ARG(factor == 1 || ((H & 1) == 0 && (W & 1) == 0), "rnerf_images_prepare: factor 2 needs even H and W, got %d x %d", H, W);
  const int h = H / factor, w = W / factor;
  // 256 output pixels per block, the block index in 31 bits; n H W C itself may well exceed 2^31 (a few hundred full-HD views do)
  RNERF_CHECK_ARG(n <= ((1LL << 39) - 256) / ((long long)h * w), "rnerf_images_prepare: n * (H / factor) * (W / factor) must be below 2^39");
  RNERF_CHECK_ARG(C == 3 || ((uintptr_t)src & 3) == 0, "rnerf_images_prepare: RGBA src must be 4-byte aligned");
  RNERF_CHECK_ARG(((uintptr_t)dst & 3) == 0, "rnerf_images_prepare: dst must be 4-byte aligned");
  const long long total = (long long)n * h * w;
  hipStream_t st = (hipStream_t)stream;
  if (C == 4) {
    if (factor == 1) {
      if (white_bkgd) launch_images_prepare<4, 1, true>(src, total, w, dst, st);
      else launch_images_prepare<4, 1, false>(src, total, w, dst, st);
    } else {
      if (white_bkgd) launch_images_prepare<4, 2, true>(src, total, w, dst, st);
      else launch_images_prepare<4, 2, false>(src, total, w, dst, st);
    }
  } else {
    if (factor == 1) launch_images_prepare<3, 1, false>(src, total, w, dst, st);
    else launch_images_prepare<3, 2, false>(src, total, w, dst, st);
  }
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}
