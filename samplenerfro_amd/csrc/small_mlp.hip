// The small MLPs in exact fp32 on the matrix cores (N2) and the stage "all*" kernels built on them: so3_mlp's evaluation, the march that
// uses it, the background MLP's and so3_mlp's backward, the adjoint of the march.  Nothing here is shared with the NerfMLP engines
// (csrc/mlp.hip); the f16 hi + lo training forwards of the same two networks live in csrc/bkgd16.hip.
#include "common.h"
#include "mfma_ops.h"
#include "bkgd_layout.h"
#include "so3_layout.h"

#include <type_traits>

namespace rnerf {

// ------------------------------------------------------------------------------------------------------------------
// N2: the 4x128 background MLP (rnerf/models.py:116-118) and so3_mlp in exact fp32 on v_mfma_f32_32x32x2_f32: the building blocks of
// so3_eval and of the backward kernels below (the background MLP's forward runs on the f16 matrix cores: csrc/bkgd16.hip).
// One wave = 32 rows; weights are read straight from the flat fp32 buffer (kernel[in][out], coalesced along out).
// ------------------------------------------------------------------------------------------------------------------
// acc[t] += W(step, t) * x(step) over NSTEP K=2 steps of v_mfma_f32_32x32x2_f32 for NT n-tiles, with the per-lane weight dwords fetched one
// BATCH (4 steps) ahead of the MFMAs that consume them.  Left to itself hipcc emits load -> s_waitcnt vmcnt(0) -> MFMA for every single
// product, re-using one register: a full L2 round trip (~650 cycles) per 64-cycle MFMA — the small-MLP kernels ran at a tenth of the
// matrix rate (the so3 training forward: 1.77 ms for 208 k rows).  wload(step, t) must be a pure load of a lane-dependent address, x(step) a
// register operand; both are called with constants after unrolling.  Same products in the same order: same bits.
template <int NSTEP, int NT, typename WF, typename XF>
__device__ __forceinline__ void mfma_f32_stream(f32x16* acc, WF wload, XF xop) {
  constexpr int BS = 4, NB = (NSTEP + BS - 1) / BS;
  float w[2][BS * NT];
#pragma unroll
  for (int i = 0; i < BS; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t) w[0][i * NT + t] = i < NSTEP ? wload(i, t) : 0.f;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (b + 1 < NB) {
#pragma unroll
      for (int i = 0; i < BS; ++i)
#pragma unroll
        for (int t = 0; t < NT; ++t) w[(b + 1) & 1][i * NT + t] = (b + 1) * BS + i < NSTEP ? wload((b + 1) * BS + i, t) : 0.f;
    }
    RNERF_PIN();
#pragma unroll
    for (int i = 0; i < BS; ++i) {
      if (b * BS + i < NSTEP) {
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[b & 1][i * NT + t], xop(b * BS + i), acc[t], 0, 0, 0);
      }
    }
    RNERF_PIN();
  }
}

// The same with the weights of a batch's 4 steps in ONE 16-byte load per n-tile (wload4(batch, t)): for the transposed products of the
// dgrad chains a lane's 4 consecutive steps read 4 consecutive floats of one kernel row, while the lanes of a load are 512 bytes apart
// (64 cache lines per instruction: the address unit, not the matrix pipe, paced these kernels with one dword per load).
template <int NSTEP, int NT, typename WF4, typename XF>
__device__ __forceinline__ void mfma_f32_stream4(f32x16* acc, WF4 wload4, XF xop) {
  static_assert(NSTEP % 4 == 0, "whole batches");
  constexpr int NB = NSTEP / 4;
  float4 w[2][NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) w[0][t] = wload4(0, t);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (b + 1 < NB) {
#pragma unroll
      for (int t = 0; t < NT; ++t) w[(b + 1) & 1][t] = wload4(b + 1, t);
    }
    RNERF_PIN();
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float4 q = w[b & 1][t];
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(i == 0 ? q.x : (i == 1 ? q.y : (i == 2 ? q.z : q.w)), xop(4 * b + i), acc[t], 0, 0, 0);
      }
    RNERF_PIN();
  }
}

__device__ __forceinline__ void small_init_bias(f32x16 (&acc)[4], const float* __restrict__ bias, int h) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = bias[32 * t + (r & 3) + 8 * (r >> 2) + 4 * h];
}

// acc += W[rows f(h)][:] x operand, for the 64 (t,r) steps of a 128-wide previous activation held in `x`
__device__ __forceinline__ void small_prev_layer(f32x16 (&acc)[4], const f32x16 (&x)[4], const float* __restrict__ kern, int m, int h) {
  const float* __restrict__ kl = kern + 4 * h * 128 + m;           // step (ts, r): the feature this half holds in x[ts][r] = 32 ts + (r & 3) + 8 (r >> 2) + 4 h
  mfma_f32_stream<64, 4>(acc, [&](int st, int t) { return kl[(32 * (st >> 4) + (st & 3) + 8 * ((st & 15) >> 2)) * 128 + 32 * t]; },
                         [&](int st) { return x[st >> 4][st & 15]; });
}

// ------------------------------------------------------------------------------------------------------------------
// G4 / P2 / E1 (stage "all"): so3_mlp = MLP(128, 4, skip 2, out 3) on annealed_pos_enc(x) (rnerf/ior_utils.py:148-152, :283;
// rnerf/model_utils.py:236-245), the Rodrigues rotation of grad n by that axis-angle (ior_utils.py:305-312), and the march
// that uses it (rnerf/eikonal_utils.py:34-39).  Same exact-fp32 MFMA chain as the background MLP; one wave = 32 points.
// ------------------------------------------------------------------------------------------------------------------
// K=2 steps over the 60 annealed features: step p, half h -> feature 2p + h = 6d + 3*is_cos + c with d = p / 3 for both halves
__device__ __forceinline__ void so3_enc_layer(f32x16 (&acc)[4], const float (&enc)[30], const float* __restrict__ kern, int m, int h) {
  const float* __restrict__ kl = kern + h * 128 + m;
  mfma_f32_stream<30, 4>(acc, [&](int p, int t) { return kl[2 * p * 128 + 32 * t]; }, [&](int p) { return enc[p]; });
}

// raw axis-angle of one point per lane pair (lanes m and m + 32 hold the same point); all 64 lanes must call it
__device__ __forceinline__ void so3_eval(const float* __restrict__ params, float px, float py, float pz, const So3Window& win, int m, int h,
                                         float (&raw)[3]) {
  float enc[30];
  const float HALF_PI = 1.5707963705062866f;
#pragma unroll
  for (int p = 0; p < 30; ++p) {
    const int d = p / 3, k = p % 3;
    const float x = k == 0 ? (h ? py : px) : (k == 1 ? (h ? px : pz) : (h ? pz : py));
    const float phase = k == 0 ? 0.f : (k == 1 ? (h ? HALF_PI : 0.f) : HALF_PI);
    const float xb = fmul(x, (float)(1 << d));
    enc[p] = fmul(sinf(k == 0 ? xb : fadd(xb, phase)), win.w[d]);
  }
  f32x16 acc[4], x[4];
  small_init_bias(acc, params + so3_boff(0), h);
  so3_enc_layer(acc, enc, params + so3_koff(0), m, h);
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) x[t][r] = fmaxf(acc[t][r], 0.f);
#pragma unroll 1
  for (int l = 1; l <= 2; ++l) {
    small_init_bias(acc, params + (l == 1 ? so3_boff(1) : so3_boff(2)), h);
    small_prev_layer(acc, x, params + (l == 1 ? so3_koff(1) : so3_koff(2)), m, h);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) x[t][r] = fmaxf(acc[t][r], 0.f);
  }
  small_init_bias(acc, params + so3_boff(3), h);                     // Dense_3: [x(128), inputs(60)] (skip concat after i == 2)
  small_prev_layer(acc, x, params + so3_koff(3), m, h);
  so3_enc_layer(acc, enc, params + so3_koff(3) + 128 * 128, m, h);
  float o[3] = {0.f, 0.f, 0.f};
  const float* __restrict__ k4 = params + so3_koff(4);
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = fmaxf(acc[t][r], 0.f);
      const int f = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
      o[0] = fmaf(v, k4[f * 3 + 0], o[0]); o[1] = fmaf(v, k4[f * 3 + 1], o[1]); o[2] = fmaf(v, k4[f * 3 + 2], o[2]);
    }
#pragma unroll
  for (int c = 0; c < 3; ++c) raw[c] = o[c] + __shfl_xor(o[c], 32) + params[so3_boff(4) + c];
}

// ---- so3_mlp on the 16-bit matrix cores (f16 hi + lo split of both operands, 3 MFMAs per product tile, fp32 accumulate: the arithmetic of
// the NerfMLP engine) for the march of stage "all*", where it runs once per node of the boundary shell.  One WORKGROUP of four waves
// evaluates it for 16 rays on v_mfma_f32_16x16x32_f16 (transposed chain: weights = A, rows = output features; activations = B, columns =
// rays): lane (ray c = lane & 15, k-group g = lane >> 4) holds D rows 4 g + i of a 16-feature tile.  Wave w owns the output tiles 2 w and
// 2 w + 1 (32 features) of every layer, so after a layer it holds, per lane, the 8 values
//     slot j < 4: feature 32 w + 4 g + j (tile 2 w)       slot j >= 4: feature 32 w + 16 + 4 g + (j - 4) (tile 2 w + 1)
// which is exactly what lane (c, g) must supply as B operand of k-step w (K = 32) of the next layer when the packed weights use the same
// slot -> feature map.  Packed stream: 16 k-steps (Dense_0: 2 encoding; Dense_1, Dense_2: 4; Dense_3: 4 + 2 encoding) x 8 tiles; block
// (ks, t) = 64 lanes x uint4 hi, then lo (2 KiB).  Encoding k-steps use feature 32 s + 8 g + j of annealed_pos_enc (zero past 59).
constexpr int kSo3KSteps = 16;
constexpr int kSo3Blocks = kSo3KSteps * 8;                       // 128 blocks x 2 KiB
constexpr float SO3_WSCALE = 256.f;                              // keeps the lo parts of the f16 split normal (as Prec<F16X3>::WSCALE)
// kernel row (input feature) of Dense_l fed by slot j of lane group g in k-step ks, or -1 (zero padding); l through *layer
__host__ __device__ constexpr int so3s_row(int ks, int g, int j, int* layer) {
  const int l = ks < 2 ? 0 : (ks < 6 ? 1 : (ks < 10 ? 2 : 3));
  const int s = ks - (l == 0 ? 0 : (l == 1 ? 2 : (l == 2 ? 6 : 10)));
  *layer = l;
  const bool enc = l == 0 || (l == 3 && s >= 4);
  if (enc) { const int f = 32 * (l == 0 ? s : s - 4) + 8 * g + j; return f < 60 ? (l == 0 ? f : 128 + f) : -1; }
  return 32 * s + (j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4));
}

__global__ void so3_pack16_kernel(const float* __restrict__ params, uint4* __restrict__ packed) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= kSo3Blocks * 64) return;
  const int blk = gid >> 6, lane = gid & 63;
  const int ks = blk >> 3, t = blk & 7;
  const int n_out = 16 * t + (lane & 15), g = lane >> 4;
  float w[8];
  for (int j = 0; j < 8; ++j) {
    int l = 0;
    const int row = so3s_row(ks, g, j, &l);
    w[j] = row < 0 ? 0.f : params[(l == 0 ? so3_koff(0) : (l == 1 ? so3_koff(1) : (l == 2 ? so3_koff(2) : so3_koff(3)))) + row * 128 + n_out] * SO3_WSCALE;
  }
  uint32_t hi[4], lo[4];
  for (int p = 0; p < 4; ++p) split2<true>(w[2 * p], w[2 * p + 1], hi[p], lo[p]);
  packed[(size_t)blk * 128 + lane] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
  packed[(size_t)blk * 128 + 64 + lane] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

struct So3Ops { uint4 h, l; };
__device__ __forceinline__ So3Ops so3_split_ops(const float (&x)[8]) {
  uint32_t hh[4], ll[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) split2<true>(x[2 * p], x[2 * p + 1], hh[p], ll[p]);
  So3Ops o; o.h = make_uint4(hh[0], hh[1], hh[2], hh[3]); o.l = make_uint4(ll[0], ll[1], ll[2], ll[3]);
  return o;
}

// LDS of one 16-ray workgroup.  Every exchange has its own region, so one barrier per exchange is enough (a region is rewritten only after
// the barriers of a whole evaluation have been passed by every wave).
struct So3Shared {
  uint4 enc[2][2][64];          // encoding operands: k-step, (hi, lo), lane
  uint4 x[3][4][2][64];         // inputs of Dense_1, Dense_2, Dense_3: k-step, (hi, lo), lane
  float4 out[4][16];            // Dense_4 partial sums per wave and ray
  float4 pos[16];               // the points to evaluate (written by the marching wave)
  float bias[4][128];           // Dense_0 .. Dense_3
  float k4[128][4];             // Dense_4 kernel rows (3 outputs, padded)
  float tail[16];               // Dense_4 bias (3), the annealing window (10) at [4..13]
  int done;                     // set by the marching wave before its last barrier
};

typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 so3_mfma16(const uint4 a, const uint4 b, const f32x4 c) {
  typedef _Float16 h8 __attribute__((ext_vector_type(8)));
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
}

__device__ __forceinline__ void so3_shared_init(So3Shared& sh, const float* __restrict__ params, const So3Window& win, int tid) {
  for (int i = tid; i < 4 * 128; i += 256) { const int l = i >> 7, n = i & 127; sh.bias[l][n] = params[(l == 0 ? so3_boff(0) : (l == 1 ? so3_boff(1) : (l == 2 ? so3_boff(2) : so3_boff(3)))) + n]; }
  for (int i = tid; i < 128 * 3; i += 256) sh.k4[i / 3][i % 3] = params[so3_koff(4) + i];
  if (tid < 3) sh.tail[tid] = params[so3_boff(4) + tid];
  if (tid < 10) sh.tail[4 + tid] = win.w[tid];
  if (tid == 0) sh.done = 0;
}

// One evaluation of so3_mlp at the 16 points sh.pos[] by the four waves of the workgroup (all must call it; 5 barriers).  Wave w keeps
// its slice of the packed stream — tiles 2 w, 2 w + 1 of the 16 k-steps, hi and lo = 256 registers — for the whole march: an evaluation
// reads no weight from memory.  Between layers the waves exchange the converted operands through LDS: wave w converts its 32 outputs
// (bias + ReLU + hi/lo split) = k-step w of the next layer; the encoding is split the same way (wave w: slots 4 (w & 1) .. + 3 of k-step
// w >> 1, four sines per lane).  All operand reads of a layer are issued ahead of its MFMAs, which alternate between the wave's two
// accumulators.  The result — Dense_4 (128 -> 3, fp32 VALU) as four 32-feature partials — is left in sh.out[wave][ray].
__device__ __forceinline__ void so3_eval_wg(So3Shared& sh, const uint4 (&wh)[kSo3KSteps][2], const uint4 (&wl)[kSo3KSteps][2], int wave, int lane) {
  const int c = lane & 15, g = lane >> 4;
  const float HALF_PI = 1.5707963705062866f;
  const f32x4 zero = {0, 0, 0, 0};
  constexpr float INV = 1.0f / SO3_WSCALE;
  const float4 pt = sh.pos[c];
  {   // annealed_pos_enc (model_utils.py:236-245): feature f = 6 d + 3 is_cos + c3, slots 4 (w & 1) .. + 3 of k-step w >> 1
    const int s = wave >> 1, j0 = 4 * (wave & 1);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int f = 32 * s + 8 * g + j0 + j;
      const bool in = f < 60;
      const int fc = in ? f : 0;
      const int d = fc / 6, jj = fc - 6 * d, c3 = jj >= 3 ? jj - 3 : jj;
      const float x = c3 == 0 ? pt.x : (c3 == 1 ? pt.y : pt.z);
      const float xb = fmul(x, (float)(1 << d));
      const float e = fmul(pe_sin(jj >= 3 ? fadd(xb, HALF_PI) : xb), sh.tail[4 + d]);     // ~1 ulp, 20 VALU ops (ocml sinf: ~100)
      v[j] = in ? e : 0.f;
    }
    uint32_t h0, l0, h1, l1;
    split2<true>(v[0], v[1], h0, l0); split2<true>(v[2], v[3], h1, l1);
    uint2* eh = (uint2*)&sh.enc[s][0][lane] + (wave & 1);
    uint2* el = (uint2*)&sh.enc[s][1][lane] + (wave & 1);
    *eh = make_uint2(h0, h1); *el = make_uint2(l0, l1);
  }
  __syncthreads();
  f32x4 a0 = zero, a1 = zero;
  auto kstep = [&](int ks, const uint4 bh, const uint4 bl) {        // hi*hi + hi*lo + lo*hi, the two tiles interleaved
    a0 = so3_mfma16(wh[ks][0], bh, a0); a1 = so3_mfma16(wh[ks][1], bh, a1);
    a0 = so3_mfma16(wh[ks][0], bl, a0); a1 = so3_mfma16(wh[ks][1], bl, a1);
    a0 = so3_mfma16(wl[ks][0], bh, a0); a1 = so3_mfma16(wl[ks][1], bh, a1);
  };
  auto enc_layer = [&](int ks0) {     // the encoding operands feed Dense_0 and, through the skip concat, Dense_3
    uint4 eh[2], el[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) { eh[s] = sh.enc[s][0][lane]; el[s] = sh.enc[s][1][lane]; }
    RNERF_PIN();
#pragma unroll
    for (int s = 0; s < 2; ++s) kstep(ks0 + s, eh[s], el[s]);
  };
  // ReLU(acc / scale + bias) of this wave's 32 outputs = the operands of k-step w of the next layer
  auto hand_over = [&](int l) {
    const float4 b0 = *(const float4*)&sh.bias[l][32 * wave + 4 * g], b1 = *(const float4*)&sh.bias[l][32 * wave + 16 + 4 * g];
    float v[8];
    v[0] = fmaxf(fmaf(a0[0], INV, b0.x), 0.f); v[1] = fmaxf(fmaf(a0[1], INV, b0.y), 0.f); v[2] = fmaxf(fmaf(a0[2], INV, b0.z), 0.f); v[3] = fmaxf(fmaf(a0[3], INV, b0.w), 0.f);
    v[4] = fmaxf(fmaf(a1[0], INV, b1.x), 0.f); v[5] = fmaxf(fmaf(a1[1], INV, b1.y), 0.f); v[6] = fmaxf(fmaf(a1[2], INV, b1.z), 0.f); v[7] = fmaxf(fmaf(a1[3], INV, b1.w), 0.f);
    const So3Ops o = so3_split_ops(v);
    sh.x[l][wave][0][lane] = o.h; sh.x[l][wave][1][lane] = o.l;
  };
  auto layer = [&](int l, int ks0) {
    uint4 bh[4], bl[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) { bh[s] = sh.x[l][s][0][lane]; bl[s] = sh.x[l][s][1][lane]; }
    RNERF_PIN();
    a0 = zero; a1 = zero;
#pragma unroll
    for (int s = 0; s < 4; ++s) kstep(ks0 + s, bh[s], bl[s]);
  };
  enc_layer(0);
  hand_over(0);
  __syncthreads();
  layer(0, 2);
  hand_over(1);
  __syncthreads();
  layer(1, 6);
  hand_over(2);
  __syncthreads();
  layer(2, 10);
  enc_layer(14);                     // skip concat (model_utils.py:131-132)
  // Dense_4 (128 -> 3) on the VALU in fp32: this wave's 32 features, 8 per lane
  float o[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int f = 32 * wave + (j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4));
    const float v = fmaxf(fmaf(j < 4 ? a0[j & 3] : a1[j & 3], INV, sh.bias[3][f]), 0.f);
    const float4 k = *(const float4*)&sh.k4[f][0];
    o[0] = fmaf(v, k.x, o[0]); o[1] = fmaf(v, k.y, o[1]); o[2] = fmaf(v, k.z, o[2]);
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) { o[q] = o[q] + __shfl_xor(o[q], 16); o[q] = o[q] + __shfl_xor(o[q], 32); }
  if (g == 0) sh.out[wave][c] = make_float4(o[0], o[1], o[2], 0.f);
  __syncthreads();
}

// pred_grad = a (cos(t) v + sin(t) e x v + (1 - cos(t)) (e . v) e),  e = raw / |raw|, v = g / |g| with safe norms (ior_utils.py:305-312)
__device__ __forceinline__ void so3_rotate(const float (&raw)[3], const float (&g)[3], float (&pred)[3]) {
  const float theta = fsqrt(fmaxf(fadd(fadd(fmul(raw[0], raw[0]), fmul(raw[1], raw[1])), fmul(raw[2], raw[2])), 1e-6f));
  const float e[3] = {fdiv(raw[0], theta), fdiv(raw[1], theta), fdiv(raw[2], theta)};
  const float a = fsqrt(fmaxf(fadd(fadd(fmul(g[0], g[0]), fmul(g[1], g[1])), fmul(g[2], g[2])), 1e-6f));
  const float v[3] = {fdiv(g[0], a), fdiv(g[1], a), fdiv(g[2], a)};
  const float ct = cosf(theta), st = sinf(theta);
  const float cr[3] = {fsub(fmul(e[1], v[2]), fmul(e[2], v[1])), fsub(fmul(e[2], v[0]), fmul(e[0], v[2])), fsub(fmul(e[0], v[1]), fmul(e[1], v[0]))};
  const float dot = fadd(fadd(fmul(e[0], v[0]), fmul(e[1], v[1])), fmul(e[2], v[2]));
  const float k = fmul(fsub(1.0f, ct), dot);
#pragma unroll
  for (int c = 0; c < 3; ++c) pred[c] = fmul(a, fadd(fadd(fmul(ct, v[c]), fmul(st, cr[c])), fmul(k, e[c])));
}

// G4: VoxMLP.__call__ for arbitrary points -> (n, grad n) and pred_grad
__global__ void __launch_bounds__(64) so3_query_kernel(const float4* __restrict__ table, GridParams gp, const float* __restrict__ params,
                                                       So3Window win, const float* __restrict__ pts, const float* __restrict__ cond, long long n,
                                                       float4* __restrict__ out4, float* __restrict__ pred_out) {
  const int lane = threadIdx.x & 63, m = lane & 31, h = lane >> 5;
  long long row = (long long)blockIdx.x * 32 + m;
  const bool ok = row < n;
  if (!ok) row = n - 1;
  const float px = pts[3 * row], py = pts[3 * row + 1], pz = pts[3 * row + 2];
  const float4 c = trilinear(table, gp, px, py, pz, nullptr);
  float raw[3], pred[3];
  so3_eval(params, px, py, pz, win, m, h, raw);
  // wrapper_grad_mlp (ior_utils.py:225-267) rotates a caller-supplied vector; VoxMLP.__call__ (:269-312) the looked-up gradient
  const float g[3] = {cond ? cond[3 * row] : c.y, cond ? cond[3 * row + 1] : c.z, cond ? cond[3 * row + 2] : c.w};
  so3_rotate(raw, g, pred);
  if (ok && h == 0) { out4[row] = c; pred_out[3 * row] = pred[0]; pred_out[3 * row + 1] = pred[1]; pred_out[3 * row + 2] = pred[2]; }
}

// E1/E2 with stage "all": one workgroup = 16 rays.  Wave 0 marches them exactly like march_kernel does — four lanes per ray (lane q owns
// coordinate q of the state and component (q + 1) & 3 of the table entries), the gathers of the next two nodes in flight from predicted
// cells — and at every node where any of its rays is inside the boundary shell (|grad n| > 1e-3) hands the 16 positions to LDS; the other
// three waves wait at that barrier, and all four evaluate so3_mlp together (so3_eval_wg).  Outside the shell a node costs what it costs in
// the radiance-stage march; inside, the chain is one evaluation of 96 v_mfma_f32_16x16x32_f16 per wave.
__global__ void __launch_bounds__(256, 1) march_all_kernel(const float4* __restrict__ table4, GridParams gp, const float* __restrict__ params,
                                                          const uint4* __restrict__ packed16, So3Window win, const float* __restrict__ origins, const float* __restrict__ viewdirs,
                                                          int B, float near, float step, int num_nodes, float4* __restrict__ path_pd4,
                                                          float4* __restrict__ path_dr4, float4* __restrict__ path_ior4,
                                                          // training record (nullable): raw direction + n per node, and the compacted list of
                                                          // (ray, node) pairs at which pred_grad was selected (the object's boundary shell)
                                                          float4* __restrict__ path_rdn4, int* __restrict__ pair_count, int pair_cap,
                                                          int2* __restrict__ pair_id, float4* __restrict__ pair_x4, float4* __restrict__ pair_g4,
                                                          int* __restrict__ pair_of_node, const int* __restrict__ ray_order) {
  __shared__ So3Shared sh;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  so3_shared_init(sh, params, win, threadIdx.x);
  uint4 wh[kSo3KSteps][2], wl[kSo3KSteps][2];
#pragma unroll
  for (int ks = 0; ks < kSo3KSteps; ++ks)
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const uint4* __restrict__ blk = packed16 + (size_t)(8 * ks + 2 * wave + tt) * 128;
      wh[ks][tt] = blk[lane]; wl[ks][tt] = blk[64 + lane];
    }
  __syncthreads();
  if (wave != 0) {                    // the evaluation waves: wait for the marcher's next request (or the end of the march)
    for (;;) {
      __syncthreads();
      if (sh.done) return;
      so3_eval_wg(sh, wh, wl, wave, lane);
    }
  }
  // ---- the marching wave: march_kernel's node (march.hip), plus the so3 term
  const float* __restrict__ table = (const float*)table4;
  float* __restrict__ path_pd = (float*)path_pd4; float* __restrict__ path_dr = (float*)path_dr4;
  float* __restrict__ path_ior = (float*)path_ior4; float* __restrict__ path_rdn = (float*)path_rdn4;
  float* __restrict__ pair_x = (float*)pair_x4; float* __restrict__ pair_g = (float*)pair_g4;
  const int q = lane & 3, ray = lane >> 2;
  int r = blockIdx.x * 16 + ray;
  const bool live = r < B;
  if (!live) r = B - 1;               // surplus quads replay the last ray (same values to the same addresses); their pair records are suppressed
  if (ray_order) r = ray_order[r];    // the rays of a workgroup in the caller's (shell-coherent) order; records go to the ray's own index
  const int qc = q < 3 ? q : 0;
  const float nmin_q = qc == 0 ? gp.nminx : (qc == 1 ? gp.nminy : gp.nminz);
  const double rcp_q = 1.0 / (double)(qc == 0 ? gp.ndx : (qc == 1 ? gp.ndy : gp.ndz));
  const int dim_q = qc == 0 ? gp.dx : (qc == 1 ? gp.dy : gp.dz);
  const unsigned comp = (q + 1) & 3;
  const char* __restrict__ tabc = (const char*)table;
  const unsigned cofs = comp * 4u;
  const unsigned sa_q = gp.sa[qc], sb_q = gp.sb[qc];                // table addressing of this lane's axis, either layout (GridParams::sa / sb)
  const int hi_q = dim_q - 1;
  float d = q < 3 ? viewdirs[3 * r + qc] : 0.f;
  float p = q < 3 ? fadd(origins[3 * r + qc], fmul(near, d)) : 0.f;   // eikonal_utils.py:104-106
  float rt = near;
  struct Corners { float c[8]; int i0, i1; };     // 000 100 001 101 010 110 011 111 (xyz) + the indices they were gathered with
  Corners ca, cb, cc;
  auto gather = [&](int i0, int i1, Corners& o) {       // (the integer glue as in march.hip: clamp0 / floor_to_int / lerp_pk, common.h)
    o.i0 = i0; o.i1 = i1;
    const unsigned m0 = __umul24((unsigned)i0 >> 1, sa_q) + __umul24((unsigned)i0 & 1u, sb_q);
    const unsigned m1 = __umul24((unsigned)i1 >> 1, sa_q) + __umul24((unsigned)i1 & 1u, sb_q);
    const unsigned y0 = quad_bcast_i<1>(m0), y1 = quad_bcast_i<1>(m1);
    const unsigned z0 = quad_bcast_i<2>(m0) + cofs, z1 = quad_bcast_i<2>(m1) + cofs;
    const unsigned b00 = quad_bcast_i<0>(m0) + y0, b10 = quad_bcast_i<0>(m1) + y0, b01 = quad_bcast_i<0>(m0) + y1, b11 = quad_bcast_i<0>(m1) + y1;
    o.c[0] = *(const float*)(tabc + (b00 + z0)); o.c[1] = *(const float*)(tabc + (b10 + z0));
    o.c[2] = *(const float*)(tabc + (b00 + z1)); o.c[3] = *(const float*)(tabc + (b10 + z1));
    o.c[4] = *(const float*)(tabc + (b01 + z0)); o.c[5] = *(const float*)(tabc + (b11 + z0));
    o.c[6] = *(const float*)(tabc + (b01 + z1)); o.c[7] = *(const float*)(tabc + (b11 + z1));
  };
  auto predict = [&](float xq, Corners& o) {
    const int j = floor_to_int(xq);
    gather(clamp0(j, hi_q), clamp0(j + 1, hi_q), o);
  };
  float x_prev;
  {
    const float x = div_const(fsub(p, nmin_q), rcp_q);
    x_prev = div_const(fsub(fsub(p, fmul(step, d)), nmin_q), rcp_q);   // as if a vacuum step had led here
    predict(x, ca);
    predict(fadd(x, fsub(x, x_prev)), cb);
  }
  const size_t node_stride = 4 * (size_t)B;
  size_t rec = 4 * (size_t)r;                                           // float offset of this ray's record of the current node
  auto one_step = [&](int k, Corners& cn, Corners& nx) {
    // ---- VoxMLP._linear3 addressing (ior_utils.py:188-211): one coordinate per lane
    const float x = div_const(fsub(p, nmin_q), rcp_q);
    const float fx = floorf(x);
    const int i = (int)fx;
    const float t = fsub(x, fx);
    const int i0 = clamp0(i, hi_q), i1 = clamp0(i + 1, hi_q);
    if (__builtin_amdgcn_ballot_w64(i0 != cn.i0 || i1 != cn.i1) != 0) gather(i0, i1, cn);     // mispredicted somewhere in the wave
    const float dx = fsub(x, x_prev);
    predict(fadd(x, fadd(dx, dx)), nx);
    x_prev = x;
    const float xd = quad_bcast<0>(t), yd = quad_bcast<1>(t), zd = quad_bcast<2>(t);
    // ---- node record while the gathers are in flight (eikonal_utils.py:112-114), direction safe-normalised (math_utils.py:6-12)
    const float nrm = fsqrt(fmaxf(quad_sumsq3(d), 1e-6f));
    path_pd[rec + q] = q < 3 ? p : rt;
    path_dr[rec + q] = q < 3 ? fdiv(d, nrm) : 0.f;
    // ---- 7 lerps a*(1-t) + b*t (ior_utils.py:214-222)
    const f32x2_t wx = {fsub(1.0f, xd), xd}, wy = {fsub(1.0f, yd), yd}, wz = {fsub(1.0f, zd), zd};
    const float c00 = lerp_pk(cn.c[0], cn.c[1], wx);
    const float c01 = lerp_pk(cn.c[2], cn.c[3], wx);
    const float c10 = lerp_pk(cn.c[4], cn.c[5], wx);
    const float c11 = lerp_pk(cn.c[6], cn.c[7], wx);
    const float c0 = lerp_pk(c00, c10, wy);
    const float c1 = lerp_pk(c01, c11, wy);
    const float c = lerp_pk(c0, c1, wz);   // lanes 0..2: grad component q, lane 3: n
    if (path_ior) path_ior[rec + comp] = c;
    const float n = quad_bcast<3>(c);
    const float s = fdiv(step, n);
    const float np = fadd(p, fmul(s, d));                // needs the current direction only
    // |grad n| > 1e-3 (eikonal_utils.py:35): sqrt_rn(s) > f32(1e-3) <=> s > 0x358637BE, the largest f32 whose correctly rounded root is
    // still <= f32(1e-3) (sqrt is monotone): the same decision for every s without a root on the chain
    const float g2 = quad_sumsq3(c);
    const bool use = g2 > __uint_as_float(0x358637BEu);
    int idx = -1;
    if (path_rdn) {
      path_rdn[rec + q] = q < 3 ? d : n;
      if (use && q == 0 && live) idx = atomicAdd(pair_count, 1);      // consumed after the evaluation: its round trip hides behind the MLP
    }
    float pred = 0.f;
    if (__builtin_amdgcn_ballot_w64(use) != 0) {         // (a workgroup's rays are neighbours in the shell-coherent order)
      if (q < 3) ((float*)&sh.pos[ray])[q] = p;
      __syncthreads();
      so3_eval_wg(sh, wh, wl, 0, lane);
      const float4 r0 = sh.out[0][ray], r1 = sh.out[1][ray], r2 = sh.out[2][ray], r3 = sh.out[3][ray];
      const float o0 = q == 0 ? r0.x : (q == 1 ? r0.y : r0.z), o1 = q == 0 ? r1.x : (q == 1 ? r1.y : r1.z);
      const float o2 = q == 0 ? r2.x : (q == 1 ? r2.y : r2.z), o3 = q == 0 ? r3.x : (q == 1 ? r3.y : r3.z);
      const float raw = q < 3 ? ((o0 + o1) + (o2 + o3)) + sh.tail[qc] : 0.f;
      // pred_grad = a (cos(t) v + sin(t) e x v + (1 - cos(t)) (e . v) e),  e = raw / |raw|, v = g / |g| with safe norms (ior_utils.py:305-312)
      const float theta = fsqrt(fmaxf(quad_sumsq3(raw), 1e-6f));
      const float e = fdiv(raw, theta);
      const float a = fsqrt(fmaxf(g2, 1e-6f));
      const float v = q < 3 ? fdiv(c, a) : 0.f;
      float ct, st;
      pe_sincos(theta, st, ct);
      const float e0 = quad_bcast<0>(e), e1 = quad_bcast<1>(e), e2 = quad_bcast<2>(e);
      const float v0 = quad_bcast<0>(v), v1 = quad_bcast<1>(v), v2 = quad_bcast<2>(v);
      const float ea = q == 0 ? e1 : (q == 1 ? e2 : e0), eb = q == 0 ? e2 : (q == 1 ? e0 : e1);
      const float va = q == 0 ? v1 : (q == 1 ? v2 : v0), vb = q == 0 ? v2 : (q == 1 ? v0 : v1);
      const float cr = fsub(fmul(ea, vb), fmul(eb, va));
      const float dot = fadd(fadd(fmul(e0, v0), fmul(e1, v1)), fmul(e2, v2));
      const float kk = fmul(fsub(1.0f, ct), dot);
      pred = fmul(a, fadd(fadd(fmul(ct, v), fmul(st, cr)), fmul(kk, e)));
    }
    if (path_rdn) {
      idx = quad_bcast_i<0>(idx);
      if (idx >= pair_cap) idx = -1;
      if (idx >= 0) {
        if (q == 0) pair_id[idx] = make_int2(r, k);
        pair_x[4 * (size_t)idx + q] = q < 3 ? p : 0.f;
        pair_g[4 * (size_t)idx + q] = q < 3 ? c : 0.f;
      }
      if (q == 0 && live) pair_of_node[(size_t)k * B + r] = idx;
    }
    d = fadd(d, fmul(step, use ? pred : c));
    rt = fadd(rt, fsqrt(quad_sumsq3(fsub(p, np))));
    p = np;
    rec += node_stride;
  };
  int k = 0;
  for (; k + 2 < num_nodes; k += 3) {      // three nodes per trip: the corner register sets rotate instead of being copied
    one_step(k, ca, cc);
    one_step(k + 1, cb, ca);
    one_step(k + 2, cc, cb);
  }
  if (k < num_nodes) { one_step(k, ca, cc); ++k; }
  if (k < num_nodes) one_step(k, cb, ca);
  sh.done = 1;
  __syncthreads();
}

// ---- backward of the background MLP (exact fp32 on v_mfma_f32_32x32x2_f32, as the forward) --------------------------------
// dgrad chain: dX^T[k][row] = W[k][n] dY^T[n][row] with the accumulator registers as B operands; ReLU masks from the saved X_k.
__device__ __forceinline__ void small_prev_layer_T(f32x16 (&acc)[4], const f32x16 (&x)[4], const float* __restrict__ kern, int m, int h) {
  const float* __restrict__ kl = kern + m * 128 + 4 * h;           // step (ts, r): output feature n = 32 ts + 8 (r >> 2) + 4 h + (r & 3) held in x[ts][r]
  mfma_f32_stream4<64, 4>(acc, [&](int b, int t) { return *(const float4*)(kl + 32 * t * 128 + 32 * (b >> 2) + 8 * (b & 3)); },
                          [&](int st) { return x[st >> 4][st & 15]; });
}

// acc2[t2] += W[f = 32 t2 + m][n(h)] * x (contraction over the 128 outputs n held in x): the input-gradient GEMM of a small MLP, f < fin
__device__ __forceinline__ void small_input_T(f32x16 (&acc2)[2], const f32x16 (&x)[4], const float* __restrict__ kern, int fin, int m, int h) {
  mfma_f32_stream4<64, 2>(acc2, [&](int b, int t2) {
    const int f = 32 * t2 + m;
    const float4 w = *(const float4*)(kern + (f < fin ? f : fin - 1) * 128 + 32 * (b >> 2) + 8 * (b & 3) + 4 * h);
    return f < fin ? w : make_float4(0.f, 0.f, 0.f, 0.f);
  }, [&](int st) { return x[st >> 4][st & 15]; });
}

__global__ void __launch_bounds__(64) bkgd_dgrad_kernel(const float* __restrict__ params, const float* __restrict__ save,
                                                        const float* __restrict__ d_out, long long n, float pad_scale, float pad,
                                                        float* __restrict__ dy, float4* __restrict__ d_dirs) {
  const int lane = threadIdx.x & 63, m = lane & 31, h = lane >> 5;
  long long row = (long long)blockIdx.x * 32 + m;
  const bool ok = row < n;
  if (!ok) row = n - 1;
  const float* so = save + (size_t)n * (28 + 4 * 128) + (size_t)row * 3;
  float draw[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float sg = (so[c] + pad) / pad_scale;                       // out = sigmoid(raw) * (1+2p) - p   (rnerf/models.py:336-337)
    draw[c] = ok ? d_out[3 * row + c] * pad_scale * sg * (1.0f - sg) : 0.f;
  }
  float* dyraw = dy + (size_t)n * 4 * 128;
  if (ok && h == 0) { dyraw[4 * row] = draw[0]; dyraw[4 * row + 1] = draw[1]; dyraw[4 * row + 2] = draw[2]; dyraw[4 * row + 3] = 0.f; }
  auto Xk = [&](int k) -> const float* { return save + (size_t)n * 28 + (size_t)(k - 1) * n * 128 + (size_t)row * 128; };
  auto store_dy = [&](int k, const f32x16 (&xx)[4]) {
    if (ok) {
      float* dst = dy + (size_t)k * n * 128 + (size_t)row * 128;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *(float4*)(dst + 32 * t + 8 * g + 4 * h) = make_float4(xx[t][4 * g], xx[t][4 * g + 1], xx[t][4 * g + 2], xx[t][4 * g + 3]);
    }
  };
  auto mask_by = [&](int k, const f32x16 (&a)[4], f32x16 (&xx)[4]) {
    const float* xs = Xk(k);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 v = *(const float4*)(xs + 32 * t + 8 * g + 4 * h);
        xx[t][4 * g] = v.x > 0.f ? a[t][4 * g] : 0.f; xx[t][4 * g + 1] = v.y > 0.f ? a[t][4 * g + 1] : 0.f;
        xx[t][4 * g + 2] = v.z > 0.f ? a[t][4 * g + 2] : 0.f; xx[t][4 * g + 3] = v.w > 0.f ? a[t][4 * g + 3] : 0.f;
      }
  };
  const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  f32x16 acc[4], x[4];
  // through Dense_4 (128 -> 3) on the VALU
  const float* __restrict__ k4 = params + bkgd_koff(4);
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int f = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
      acc[t][r] = draw[0] * k4[f * 3] + draw[1] * k4[f * 3 + 1] + draw[2] * k4[f * 3 + 2];
    }
  mask_by(4, acc, x);
  store_dy(3, x);                                   // dY_3
  f32x16 denc[2] = {zero, zero};                    // d loss / d pos_enc(dir) (stage "all": the direction is a function of the so3 parameters)
  if (d_dirs) small_input_T(denc, x, params + bkgd_koff(3) + 128 * 128, 27, m, h);     // the skip-concat inputs of Dense_3
#pragma unroll 1
  for (int k = 3; k >= 1; --k) {                    // through Dense_k (only the first 128 input rows of Dense_3 carry gradient)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = zero;
    small_prev_layer_T(acc, x, params + (k == 3 ? bkgd_koff(3) : (k == 2 ? bkgd_koff(2) : bkgd_koff(1))), m, h);
    mask_by(k, acc, x);
    store_dy(k - 1, x);                             // dY_{k-1}
  }
  if (d_dirs) {
    small_input_T(denc, x, params + bkgd_koff(0), 27, m, h);
    const float* v = save + (size_t)row * 28;       // features 0..2 of the saved encoding = the direction itself
    const float dcv[3] = {v[0], v[1], v[2]};
    float gd3[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int f = (r & 3) + 8 * (r >> 2) + 4 * h;                  // [d(3) | sin(2^k d)(12) | sin(2^k d + pi/2)(12)]
      if (f < 3) gd3[f] += denc[0][r];
      else if (f < 27) {
        const int q = (f - 3) % 12, is_cos = (f - 3) / 12, d = q / 3, c = q % 3;
        const float xb = fmul(dcv[c], (float)(1 << d));
        gd3[c] = fmaf(denc[0][r], (float)(1 << d) * cosf(is_cos ? fadd(xb, 1.5707963705062866f) : xb), gd3[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) gd3[c] += __shfl_xor(gd3[c], 32);
    if (ok && h == 0) d_dirs[row] = make_float4(gd3[0], gd3[1], gd3[2], 0.f);
  }
}

// wgrad: dW[k][n] = sum_rows X[row][k] dY[row][n]; A = X (lane = k, the half picks one of 2 rows), B = dY: row-major fp32 needs
// no transposition for the K=2 MFMA.  One launch covers every (Dense_k block, k-tile) "unit"; a workgroup = 256 rows (4 waves x 64
// rows, summed through LDS) of one unit and writes its partial in flat-gradient layout; bkgd_wgrad_reduce_kernel adds them up.
struct BkgdUnit { int xk, ldx, kin, kt, dk, ldy, nout, goff, out_dim, boff; };   // xk: 0 = enc, k = X_k; dk: 0..3 = dY_k, 4 = d raw
__constant__ BkgdUnit kBkgdUnits[18] = {
    {0, 28, 27, 0, 0, 128, 128, bkgd_koff(0), 128, bkgd_boff(0)},
    {1, 128, 128, 0, 1, 128, 128, bkgd_koff(1), 128, bkgd_boff(1)}, {1, 128, 128, 1, 1, 128, 128, bkgd_koff(1), 128, -1},
    {1, 128, 128, 2, 1, 128, 128, bkgd_koff(1), 128, -1},            {1, 128, 128, 3, 1, 128, 128, bkgd_koff(1), 128, -1},
    {2, 128, 128, 0, 2, 128, 128, bkgd_koff(2), 128, bkgd_boff(2)}, {2, 128, 128, 1, 2, 128, 128, bkgd_koff(2), 128, -1},
    {2, 128, 128, 2, 2, 128, 128, bkgd_koff(2), 128, -1},            {2, 128, 128, 3, 2, 128, 128, bkgd_koff(2), 128, -1},
    {3, 128, 128, 0, 3, 128, 128, bkgd_koff(3), 128, bkgd_boff(3)}, {3, 128, 128, 1, 3, 128, 128, bkgd_koff(3), 128, -1},
    {3, 128, 128, 2, 3, 128, 128, bkgd_koff(3), 128, -1},            {3, 128, 128, 3, 3, 128, 128, bkgd_koff(3), 128, -1},
    {0, 28, 27, 0, 3, 128, 128, bkgd_koff(3) + 128 * 128, 128, -1},
    {4, 128, 128, 0, 4, 4, 3, bkgd_koff(4), 3, bkgd_boff(4)},       {4, 128, 128, 1, 4, 4, 3, bkgd_koff(4), 3, -1},
    {4, 128, 128, 2, 4, 4, 3, bkgd_koff(4), 3, -1},                  {4, 128, 128, 3, 4, 4, 3, bkgd_koff(4), 3, -1}};

// the so3 MLP (60 -> 128 x 4 with the 60 inputs concatenated before Dense_3 -> 3, rnerf/ior_utils.py:148-152) has the same unit structure
__constant__ BkgdUnit kSo3Units[20] = {
    {0, 60, 60, 0, 0, 128, 128, so3_koff(0), 128, so3_boff(0)},      {0, 60, 60, 1, 0, 128, 128, so3_koff(0), 128, -1},
    {1, 128, 128, 0, 1, 128, 128, so3_koff(1), 128, so3_boff(1)},    {1, 128, 128, 1, 1, 128, 128, so3_koff(1), 128, -1},
    {1, 128, 128, 2, 1, 128, 128, so3_koff(1), 128, -1},             {1, 128, 128, 3, 1, 128, 128, so3_koff(1), 128, -1},
    {2, 128, 128, 0, 2, 128, 128, so3_koff(2), 128, so3_boff(2)},    {2, 128, 128, 1, 2, 128, 128, so3_koff(2), 128, -1},
    {2, 128, 128, 2, 2, 128, 128, so3_koff(2), 128, -1},             {2, 128, 128, 3, 2, 128, 128, so3_koff(2), 128, -1},
    {3, 128, 128, 0, 3, 128, 128, so3_koff(3), 128, so3_boff(3)},    {3, 128, 128, 1, 3, 128, 128, so3_koff(3), 128, -1},
    {3, 128, 128, 2, 3, 128, 128, so3_koff(3), 128, -1},             {3, 128, 128, 3, 3, 128, 128, so3_koff(3), 128, -1},
    {0, 60, 60, 0, 3, 128, 128, so3_koff(3) + 128 * 128, 128, -1},   {0, 60, 60, 1, 3, 128, 128, so3_koff(3) + 128 * 128, 128, -1},
    {4, 128, 128, 0, 4, 4, 3, so3_koff(4), 3, so3_boff(4)},          {4, 128, 128, 1, 4, 4, 3, so3_koff(4), 3, -1},
    {4, 128, 128, 2, 4, 4, 3, so3_koff(4), 3, -1},                   {4, 128, 128, 3, 4, 4, 3, so3_koff(4), 3, -1}};
template <int KIND> struct SmallNet {
  static constexpr int ENC_LD = KIND == 0 ? 28 : 60, NPARAMS = KIND == 0 ? RNERF_BKGDMLP_PARAMS : RNERF_SO3MLP_PARAMS, UNITS = KIND == 0 ? 18 : 20;
  static constexpr int CHUNKS_PER_WG = KIND == 0 ? 1 : 4;      // 256-row chunks summed by one workgroup of the weight-gradient kernel (one partial each)
};

template <int KIND>
__global__ void __launch_bounds__(256) bkgd_wgrad_kernel(const float* __restrict__ save, const float* __restrict__ dy, long long n,
                                                         float* __restrict__ partial) {
  __shared__ float red[4][4][1024 + 32];            // [wave][n-tile][acc reg * 64 + lane] (+ the bias row)
  // 1-D grid, XCD-aware: workgroups are dealt round-robin to the 8 XCDs (each with its own L2), so workgroup b = 8 slot + xcd takes
  // unit slot % UNITS of chunk 8 (slot / UNITS) + xcd: the UNITS workgroups that read the same 256 rows of dY (each layer's dY by its
  // 4-5 k-tiles) run back to back on ONE XCD and share them in its L2 (with (chunk, unit) as grid (x, y) they were `chunks` workgroups
  // apart: every re-read went to memory).
  // CPW 256-row chunks per workgroup (so3: 4 — its 208 k pair rows made 813 partials of 65 411 floats, 213 MB written and read again by the
  // reduction: 0.56 + 0.10 ms of the stage-all step's tail; the background MLP keeps 1: a few dozen chunks, and the
  // default step's bits stay what they were)
  constexpr int UNITS = SmallNet<KIND>::UNITS, CPW = SmallNet<KIND>::CHUNKS_PER_WG;
  const int slot = blockIdx.x >> 3, xcd = blockIdx.x & 7;
  const int chunk = 8 * (slot / UNITS) + xcd, unit = slot % UNITS;      // (the index of the partial: CPW consecutive 256-row chunks)
  if ((long long)chunk * 256 * CPW >= n) return;
  const BkgdUnit u = KIND == 0 ? kBkgdUnits[unit] : kSo3Units[unit];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 31, h = lane >> 5;
  const float* __restrict__ X = u.xk == 0 ? save : save + (size_t)n * SmallNet<KIND>::ENC_LD + (size_t)(u.xk - 1) * n * 128;
  const float* __restrict__ dY = dy + (size_t)u.dk * n * 128;
  const int k = 32 * u.kt + m;
  const bool bias = u.boff >= 0;
  const int NT = (u.nout + 31) / 32;
  const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  f32x16 acc[4] = {zero, zero, zero, zero};
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};               // bias row: this lane's share of sum_rows dY[row][its column] (plain VALU adds)
  long long r0 = (long long)chunk * 256 * CPW + wave * 64;
  // Operand loads: unconditional, from clamped addresses, a BATCH of 8 row pairs ahead of the MFMAs that consume them, and made opaque
  // (empty asm on the loaded registers) before the row / column predicates are applied.  Without the last step hipcc turns
  // `ok ? load : 0` back into a branch around the load followed by s_waitcnt vmcnt(0): two exposed round trips per 4 MFMAs
  // (the so3 instance ran at a sixth of the matrix rate: 1.06 ms for 208 k rows).  The n-tile count and the bias row are compile-time
  // instances.  With 4 n-tiles (a 128-wide dY) n-tile nt is the columns {4 m + nt}: one 16-byte load per lane and row feeds all four MFMAs.
  const int kc = k < u.kin ? k : u.kin - 1;
  const bool kin_ok = k < u.kin;
  auto rows = [&](auto nt_c, auto bias_c) {
    constexpr int NTC = decltype(nt_c)::value;
    constexpr bool BIAS = decltype(bias_c)::value;
    constexpr int BS = 8, NB = 32 / BS;
    float av[2][BS];
    float4 bv[2][BS];
    const int mc = m < u.nout ? m : u.nout - 1;
    auto fetch = [&](int bi, int buf) {
#pragma unroll
      for (int j = 0; j < BS; ++j) {
        const long long rr = r0 + 2 * (bi * BS + j) + h;
        const size_t rc = (size_t)(rr < n ? rr : n - 1);
        av[buf][j] = X[rc * u.ldx + kc];
        if constexpr (NTC == 4) bv[buf][j] = *(const float4*)(dY + rc * 128 + 4 * m);
        else bv[buf][j].x = dY[rc * u.ldy + mc];
      }
    };
    fetch(0, 0);
#pragma unroll
    for (int bi = 0; bi < NB; ++bi) {
      if (bi + 1 < NB) fetch(bi + 1, (bi + 1) & 1);
      RNERF_PIN();
#pragma unroll
      for (int j = 0; j < BS; ++j) {
        const bool ok = r0 + 2 * (bi * BS + j) + h < n;
        float a = av[bi & 1][j];
        float4 q = bv[bi & 1][j];
        if constexpr (NTC == 4) asm volatile("" : "+v"(a), "+v"(q.x), "+v"(q.y), "+v"(q.z), "+v"(q.w));
        else asm volatile("" : "+v"(a), "+v"(q.x));
        a = (ok && kin_ok) ? a : 0.f;
        if constexpr (NTC == 4) {
          const float b[4] = {ok ? q.x : 0.f, ok ? q.y : 0.f, ok ? q.z : 0.f, ok ? q.w : 0.f};
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[nt], acc[nt], 0, 0, 0);
            if constexpr (BIAS) bsum[nt] += b[nt];
          }
        } else {
          const float b = (ok && m < u.nout) ? q.x : 0.f;
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[0], 0, 0, 0);
          if constexpr (BIAS) bsum[0] += b;
        }
      }
      RNERF_PIN();
    }
  };
  using I1 = std::integral_constant<int, 1>; using I4 = std::integral_constant<int, 4>;
#pragma unroll 1
  for (int cc = 0; cc < CPW; ++cc, r0 += 256) {
    if (cc > 0 && (long long)(chunk * CPW + cc) * 256 >= n) break;      // (workgroup-uniform)
    if (NT == 4) { if (bias) rows(I4{}, std::true_type{}); else rows(I4{}, std::false_type{}); }
    else { if (bias) rows(I1{}, std::true_type{}); else rows(I1{}, std::false_type{}); }
  }
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
    if (nt < NT) {
#pragma unroll
      for (int r = 0; r < 16; ++r) red[wave][nt][r * 64 + lane] = acc[nt][r];
      const float bs = bsum[nt] + __shfl_xor(bsum[nt], 32);        // even + odd rows
      if (h == 0) red[wave][nt][1024 + m] = bs;
    }
  __syncthreads();
  const int nt = wave;                                // wave w sums n-tile w over the 4 waves
  if (nt < NT) {
    float* pg = partial + (size_t)chunk * SmallNet<KIND>::NPARAMS;
    const int nn = NT == 4 ? 4 * m + nt : m;          // the column this lane's accumulator entries belong to
    if (nn < u.nout) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ki = 32 * u.kt + (r & 3) + 8 * (r >> 2) + 4 * h;
        const float v = red[0][nt][r * 64 + lane] + red[1][nt][r * 64 + lane] + red[2][nt][r * 64 + lane] + red[3][nt][r * 64 + lane];
        if (ki < u.kin) pg[u.goff + ki * u.out_dim + nn] = v;
      }
      if (bias && h == 0) pg[u.boff + nn] = red[0][nt][1024 + m] + red[1][nt][1024 + m] + red[2][nt][1024 + m] + red[3][nt][1024 + m];
    }
  }
}

template <int NPARAMS>
__global__ void __launch_bounds__(256) bkgd_wgrad_reduce_kernel(const float* __restrict__ partial, int chunks, float* __restrict__ grads) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= NPARAMS) return;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int c = 0;
  for (; c + 4 <= chunks; c += 4) {
    s0 += partial[(size_t)c * NPARAMS + e]; s1 += partial[(size_t)(c + 1) * NPARAMS + e];
    s2 += partial[(size_t)(c + 2) * NPARAMS + e]; s3 += partial[(size_t)(c + 3) * NPARAMS + e];
  }
  for (; c < chunks; ++c) s0 += partial[(size_t)c * NPARAMS + e];
  grads[e] += (s0 + s1) + (s2 + s3);
}

// ------------------------------------------------------------------------------------------------------------------
// Training of stage "all*" (SURVEY.md §8f N3): back-propagation through the N-step eikonal recurrence and through so3_mlp.
// Reference: rnerf/eikonal_utils.py:29-49,100-124 (the recurrence that
// jax.value_and_grad differentiates, train.py:164), rnerf/ior_utils.py:188-223 (_linear3), :269-312 (VoxMLP.__call__ + Rodrigues),
// rnerf/model_utils.py:236-245 (annealed_pos_enc), train.py:302-310 (path_sampler becomes trainable).
//
// The state of the recurrence is 6 numbers per ray, so the adjoint needs only 3x3 Jacobians per node:
//     rp' = rp + (step / n(rp)) rd          rd' = rd + step grad(rp),   grad = |g| > 1e-3 ? Rot(so3(rp), g(rp)) : g(rp)
//   lambda_p(k) = a_p(k) + lambda_p(k+1) + c_k (rd_k . lambda_p(k+1)) + step A_k^T lambda_d(k+1),   c_k = -step/n^2 dn/dx
//   lambda_d(k) = a_d(k) + lambda_d(k+1) + (step / n_k) lambda_p(k+1),                              A_k = d grad / d rp
// so the work splits into parallel passes over the (ray, node) pairs of the boundary shell — where so3 is evaluated — and one cheap
// sequential reverse scan:
//   (0) so3 training forward on the pairs' positions, three dgrad passes with unit cotangents -> J = d raw / d x (3x3 per pair);
//       so3_pair_jacobian_kernel: P = d pred / d raw, A = P J + (d pred / d g) G,  G = d g / d x of the trilinear interpolant;
//   (1) march_adjoint_kernel: the reverse scan; emits v = P^T (step lambda_d(k+1)), the cotangent of raw at every pair;
//   (2) so3 dgrad + wgrad with the cotangents v -> d loss / d so3 parameters.
// a_p / a_d come from nerfmlp_input_grad_kernel in csrc/mlp.hip (d loss / d position and direction of every coarse sample: through the
// position / view encodings of Dense_0, the skip concat of Dense_5 and the view layer Dense_10) and from the background MLP's input gradient.
// ------------------------------------------------------------------------------------------------------------------
// ---- so3 MLP backward, exact fp32 on v_mfma_f32_32x32x2_f32 like the background MLP's -------------------------------------------------
// (the training forward is the f16 hi + lo one of csrc/bkgd16.hip; layouts + so3_encode: csrc/so3_layout.h)
// dgrad chain of the so3 MLP + the gradient w.r.t. the input point.  Row `row` of the batch uses the saved activations of row
// `row % n_save` (the Jacobian pass runs the three unit cotangents of every point as one batch of 3 n_save rows).
__global__ void __launch_bounds__(64) so3_dgrad_kernel(const float* __restrict__ params, So3Window win, const float4* __restrict__ pts,
                                                       const float* __restrict__ save, long long n_save, const float4* __restrict__ d_raw,
                                                       long long nb, float* __restrict__ dy, float4* __restrict__ dx_out) {
  const int lane = threadIdx.x & 63, m = lane & 31, h = lane >> 5;
  long long row = (long long)blockIdx.x * 32 + m;
  const bool ok = row < nb;
  if (!ok) row = nb - 1;
  const long long srow = row % n_save;
  const float4 dr4 = d_raw[row];
  const float draw[3] = {ok ? dr4.x : 0.f, ok ? dr4.y : 0.f, ok ? dr4.z : 0.f};
  // dy == nullptr (the Jacobian passes: only d x is wanted): the dY planes, which only the wgrad reads, are not written (2 KB per row);
  // dx_out == nullptr (the parameter-gradient pass): the two input-gradient products are skipped
  float* dyraw = dy + (size_t)nb * 4 * 128;
  if (dy && ok && h == 0) *(float4*)(dyraw + 4 * row) = make_float4(draw[0], draw[1], draw[2], 0.f);
  auto store_dy = [&](int k, const f32x16 (&xx)[4]) {
    if (dy && ok) {
      float* dst = dy + (size_t)k * nb * 128 + (size_t)row * 128;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *(float4*)(dst + 32 * t + 8 * g + 4 * h) = make_float4(xx[t][4 * g], xx[t][4 * g + 1], xx[t][4 * g + 2], xx[t][4 * g + 3]);
    }
  };
  auto mask_by = [&](int k, const f32x16 (&a)[4], f32x16 (&xx)[4]) {      // ReLU': the layer's 128 sign bits (one 16-byte load per row)
    const uint4 mk = so3_load_mask(save, n_save, srow, k);
    const uint32_t w[4] = {mk.x >> (4 * h), mk.y >> (4 * h), mk.z >> (4 * h), mk.w >> (4 * h)};
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) xx[t][r] = ((w[t] >> ((r & 3) + 8 * (r >> 2))) & 1u) ? a[t][r] : 0.f;
  };
  const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  f32x16 acc[4], x[4], denc[2] = {zero, zero};
  const float* __restrict__ k4 = params + so3_koff(4);
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int f = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
      acc[t][r] = draw[0] * k4[f * 3] + draw[1] * k4[f * 3 + 1] + draw[2] * k4[f * 3 + 2];
    }
  mask_by(4, acc, x);
  store_dy(3, x);                                                                       // dY_3
  if (dx_out) small_input_T(denc, x, params + so3_koff(3) + 128 * 128, 60, m, h);       // the skip-concat inputs of Dense_3
#pragma unroll 1
  for (int k = 3; k >= 1; --k) {
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = zero;
    small_prev_layer_T(acc, x, params + (k == 3 ? so3_koff(3) : (k == 2 ? so3_koff(2) : so3_koff(1))), m, h);
    mask_by(k, acc, x);
    store_dy(k - 1, x);                                                                 // dY_{k-1}
  }
  if (!dx_out) return;
  small_input_T(denc, x, params + so3_koff(0), 60, m, h);                               // Dense_0
  // d enc -> d x through annealed_pos_enc: feature f = 6 d + 3 is_cos + c = w_d sin(2^d x_c [+ pi/2])
  const float4 pt = pts[srow];
  const float pc[3] = {pt.x, pt.y, pt.z};
  float dx[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int f = 32 * t2 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (f < 60) {
        const int d = f / 6, j = f % 6, c = j % 3;
        const float xb = fmul(pc[c], (float)(1 << d));
        const float arg = j >= 3 ? fadd(xb, 1.5707963705062866f) : xb;
        dx[c] = fmaf(denc[t2][r], win.w[d] * (float)(1 << d) * pe_cos(arg), dx[c]);
      }
    }
#pragma unroll
  for (int c = 0; c < 3; ++c) dx[c] += __shfl_xor(dx[c], 32);
  if (ok && h == 0 && dx_out) dx_out[row] = make_float4(dx[0], dx[1], dx[2], 0.f);
}

// ---- forward-mode duals for the Rodrigues rotation: value + 6 partials (d/d raw_0..2, d/d g_0..2) -----------------------------------
struct Dual6 {
  float v, d[6];
};
__device__ __forceinline__ Dual6 dmake(float v, int idx) { Dual6 r; r.v = v; for (int i = 0; i < 6; ++i) r.d[i] = i == idx ? 1.f : 0.f; return r; }
__device__ __forceinline__ Dual6 dconst(float v) { Dual6 r; r.v = v; for (int i = 0; i < 6; ++i) r.d[i] = 0.f; return r; }
__device__ __forceinline__ Dual6 operator+(const Dual6& a, const Dual6& b) { Dual6 r; r.v = a.v + b.v; for (int i = 0; i < 6; ++i) r.d[i] = a.d[i] + b.d[i]; return r; }
__device__ __forceinline__ Dual6 operator-(const Dual6& a, const Dual6& b) { Dual6 r; r.v = a.v - b.v; for (int i = 0; i < 6; ++i) r.d[i] = a.d[i] - b.d[i]; return r; }
__device__ __forceinline__ Dual6 operator*(const Dual6& a, const Dual6& b) { Dual6 r; r.v = a.v * b.v; for (int i = 0; i < 6; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i]; return r; }
__device__ __forceinline__ Dual6 operator/(const Dual6& a, const Dual6& b) {
  Dual6 r; r.v = a.v / b.v; const float inv = 1.0f / b.v;
  for (int i = 0; i < 6; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) * inv;
  return r;
}
// safe_l2_norm (rnerf/math_utils.py:6-8): sqrt(max(sum x^2, 1e-6)); the gradient of the clamped branch is zero
__device__ __forceinline__ Dual6 dsafe_norm(const Dual6 (&x)[3]) {
  const Dual6 s = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
  Dual6 r;
  if (s.v > 1e-6f) { r.v = sqrtf(s.v); const float k = 0.5f / r.v; for (int i = 0; i < 6; ++i) r.d[i] = k * s.d[i]; }
  else { r.v = sqrtf(1e-6f); for (int i = 0; i < 6; ++i) r.d[i] = 0.f; }
  return r;
}
__device__ __forceinline__ Dual6 dcos(const Dual6& a) { Dual6 r; r.v = cosf(a.v); const float k = -sinf(a.v); for (int i = 0; i < 6; ++i) r.d[i] = k * a.d[i]; return r; }
__device__ __forceinline__ Dual6 dsin(const Dual6& a) { Dual6 r; r.v = sinf(a.v); const float k = cosf(a.v); for (int i = 0; i < 6; ++i) r.d[i] = k * a.d[i]; return r; }

// value and position gradient of the trilinear interpolant (rnerf/ior_utils.py:188-223; floor() carries no gradient, the weights
// xd, yd, zd are taken before clamping): dc[a] = d c / d p_a for the 4 channels
__device__ __forceinline__ float4 trilinear_grad_finish(const TriCell& c, const GridParams& g, float4 (&dc)[3]) {
  const float ox = 1.0f - c.xd, oy = 1.0f - c.yd, oz = 1.0f - c.zd;
  auto lerp = [](const float4 a, const float4 b, float wa, float wb) { return make_float4(a.x * wa + b.x * wb, a.y * wa + b.y * wb, a.z * wa + b.z * wb, a.w * wa + b.w * wb); };
  auto sub = [](const float4 a, const float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); };
  auto scale = [](const float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); };
  // d/dx: differences along x, interpolated in y then z
  const float4 ex = lerp(lerp(sub(c.d100, c.d000), sub(c.d110, c.d010), oy, c.yd), lerp(sub(c.d101, c.d001), sub(c.d111, c.d011), oy, c.yd), oz, c.zd);
  const float4 ey = lerp(lerp(sub(c.d010, c.d000), sub(c.d110, c.d100), ox, c.xd), lerp(sub(c.d011, c.d001), sub(c.d111, c.d101), ox, c.xd), oz, c.zd);
  const float4 ez = lerp(lerp(sub(c.d001, c.d000), sub(c.d101, c.d100), ox, c.xd), lerp(sub(c.d011, c.d010), sub(c.d111, c.d110), ox, c.xd), oy, c.yd);
  dc[0] = scale(ex, 1.0f / g.ndx); dc[1] = scale(ey, 1.0f / g.ndy); dc[2] = scale(ez, 1.0f / g.ndz);
  return trilinear_finish(c);
}
__device__ __forceinline__ float4 trilinear_grad(const float4* __restrict__ tab, const GridParams& g, float px, float py, float pz, float4 (&dc)[3]) {
  TriCell c;
  trilinear_load(tab, g, px, py, pz, nullptr, c);
  return trilinear_grad_finish(c, g, dc);
}

// phase 0 (last part): per shell pair, A = d grad / d rp (3x3, row i = component of grad, column j = position axis) and
// P = d pred / d raw (3x3).  raw: so3 output (save tail), J[j]: d raw_j / d x from the three unit-cotangent dgrad passes.
__global__ void __launch_bounds__(256) so3_pair_jacobian_kernel(const float4* __restrict__ table, GridParams gp, const float4* __restrict__ pair_x,
                                                                const float4* __restrict__ pair_g, const float4* __restrict__ raw,
                                                                const float4* __restrict__ J, long long np, float* __restrict__ A, float* __restrict__ P) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  const float4 x = pair_x[i], g4 = pair_g[i], r4 = raw[i];
  Dual6 rw[3] = {dmake(r4.x, 0), dmake(r4.y, 1), dmake(r4.z, 2)};
  Dual6 gg[3] = {dmake(g4.x, 3), dmake(g4.y, 4), dmake(g4.z, 5)};
  const Dual6 theta = dsafe_norm(rw);                               // rnerf/ior_utils.py:305-312
  const Dual6 e[3] = {rw[0] / theta, rw[1] / theta, rw[2] / theta};
  const Dual6 a = dsafe_norm(gg);
  const Dual6 v[3] = {gg[0] / a, gg[1] / a, gg[2] / a};
  const Dual6 ct = dcos(theta), st = dsin(theta);
  const Dual6 cr[3] = {e[1] * v[2] - e[2] * v[1], e[2] * v[0] - e[0] * v[2], e[0] * v[1] - e[1] * v[0]};
  const Dual6 dot = e[0] * v[0] + e[1] * v[1] + e[2] * v[2];
  const Dual6 k = (dconst(1.0f) - ct) * dot;
  Dual6 pred[3];
  for (int c = 0; c < 3; ++c) pred[c] = a * (ct * v[c] + st * cr[c] + k * e[c]);
  float4 dc[3];
  trilinear_grad(table, gp, x.x, x.y, x.z, dc);
  // G[c][ax] = d g_c / d p_ax : channels y, z, w of dc[ax]
  const float G[3][3] = {{dc[0].y, dc[1].y, dc[2].y}, {dc[0].z, dc[1].z, dc[2].z}, {dc[0].w, dc[1].w, dc[2].w}};
  const float4 J0 = J[i], J1 = J[np + i], J2 = J[2 * np + i];       // J_j = d raw_j / d x (row j)
  const float Jm[3][3] = {{J0.x, J0.y, J0.z}, {J1.x, J1.y, J1.z}, {J2.x, J2.y, J2.z}};
  for (int c = 0; c < 3; ++c)
    for (int ax = 0; ax < 3; ++ax) {
      float s = 0.f;
      for (int q = 0; q < 3; ++q) s += pred[c].d[q] * Jm[q][ax] + pred[c].d[3 + q] * G[q][ax];
      A[(size_t)i * 12 + 3 * c + ax] = s;
      P[(size_t)i * 12 + 3 * c + ax] = pred[c].d[ax];               // d pred_c / d raw_ax
    }
}

// phase 1: the reverse scan of the march.  a_pos / a_dir: d loss / d (position, NORMALISED direction) of every coarse sample,
// float4[S][B] (sample-major like the rows); sample_of_node: int[N], -1 where the node is not a coarse sample.
// FOUR LANES PER RAY, as in the march: lane q < 3 owns component q of the adjoint state, of the recorded position / direction and row q
// of the 3 x 3 matrices (A = d grad / d x, P = d pred / d raw, or G = d g / d x from the table: the channel (q + 1) & 3 a lane gathers IS
// that row); lane 3 owns n and its gradient.  The matrix-transpose-vector products and the dot products run through quad broadcasts in
// the scalar formulation's association — same bits as one lane per ray, a third of the dependent instructions, four times the waves.
// Only the arithmetic of a node depends on the adjoint state; every address is known from the recorded path.  So the loads run two
// stages ahead of the arithmetic: stage A of node k - 3 (its record: position, raw direction + n, pair index), stage B of node k - 2
// (the 8 corner gathers at the recorded position, the pair's Jacobians, the sample's cotangents), arithmetic of node k.  The register
// sets rotate through an unrolled trip of 12 nodes (4 A sets x 3 B sets) instead of being copied — a copy would wait for its loads.
// (One lane per ray and one dependent round trip per stage: 2.3 us per node, 3.5 ms per 4096 x 1536 scan; pipelined: 1.7 ms.)
struct AdjNodeA { float pd, rdn; int pr; };
struct AdjNodeB { float c[8], t, A[3], P[3], ap, ad; int s; };

__global__ void __launch_bounds__(64) march_adjoint_kernel(const float4* __restrict__ table4, GridParams gp, const float4* __restrict__ path_pd4,
                                                           const float4* __restrict__ path_rdn4, const int* __restrict__ pair_of_node,
                                                           const float* __restrict__ A, const float* __restrict__ P, const float4* __restrict__ a_pos4,
                                                           const float4* __restrict__ a_dir4, const int* __restrict__ sample_of_node, int B,
                                                           int num_nodes, float step, float4* __restrict__ v_out4) {
  const float* __restrict__ path_pd = (const float*)path_pd4; const float* __restrict__ path_rdn = (const float*)path_rdn4;
  const float* __restrict__ a_pos = (const float*)a_pos4; const float* __restrict__ a_dir = (const float*)a_dir4;
  float* __restrict__ v_out = (float*)v_out4;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int q = gid & 3;
  int r = gid >> 2;
  const bool live = r < B;
  if (!live) r = B - 1;                                                // surplus quads replay the last ray, their stores are suppressed
  const int qc = q < 3 ? q : 0;
  const float nmin_q = qc == 0 ? gp.nminx : (qc == 1 ? gp.nminy : gp.nminz);
  const float nd_q = qc == 0 ? gp.ndx : (qc == 1 ? gp.ndy : gp.ndz);
  const int dim_q = qc == 0 ? gp.dx : (qc == 1 ? gp.dy : gp.dz);
  const float rnx = 1.0f / gp.ndx, rny = 1.0f / gp.ndy, rnz = 1.0f / gp.ndz;
  const unsigned comp = (q + 1) & 3;
  const unsigned sa_q = gp.sa[qc], sb_q = gp.sb[qc];                   // table addressing of this lane's axis, either layout
  const char* __restrict__ tabc = (const char*)table4;
  const unsigned cofs = comp * 4u;
  float lp = 0.f, ld = 0.f;                                            // adjoints of (rp_q, rd_q) of node k + 1 (lane 3: unused zeros)
  auto sum3 = [](float a) { return (quad_bcast<0>(a) + quad_bcast<1>(a)) + quad_bcast<2>(a); };
  auto load_a = [&](int k, AdjNodeA& a) {
    const size_t o = (size_t)k * B + r;
    a.pd = path_pd[4 * o + q]; a.rdn = path_rdn[4 * o + q]; a.pr = pair_of_node[o];
  };
  auto load_b = [&](int k, const AdjNodeA& a, AdjNodeB& b) {
    // VoxMLP._linear3 addressing (ior_utils.py:188-211), one coordinate per lane (lane 3 repeats x; its indices are not used)
    const float x = fdiv(fsub(a.pd, nmin_q), nd_q);
    const float fx = floorf(x);
    const int i = (int)fx;
    b.t = fsub(x, (float)i);
    const int i0 = clampi(i, 0, dim_q - 1), i1 = clampi(i + 1, 0, dim_q - 1);
    const unsigned m0 = ((unsigned)i0 >> 1) * sa_q + ((unsigned)i0 & 1u) * sb_q, m1 = ((unsigned)i1 >> 1) * sa_q + ((unsigned)i1 & 1u) * sb_q;
    const unsigned y0 = quad_bcast_i<1>(m0), y1 = quad_bcast_i<1>(m1);
    const unsigned z0 = quad_bcast_i<2>(m0) + cofs, z1 = quad_bcast_i<2>(m1) + cofs;
    const unsigned bx0 = quad_bcast_i<0>(m0), bx1 = quad_bcast_i<0>(m1);
    const unsigned b00 = bx0 + y0, b10 = bx1 + y0, b01 = bx0 + y1, b11 = bx1 + y1;
    b.c[0] = *(const float*)(tabc + (b00 + z0)); b.c[1] = *(const float*)(tabc + (b10 + z0));      // 000 100
    b.c[2] = *(const float*)(tabc + (b00 + z1)); b.c[3] = *(const float*)(tabc + (b10 + z1));      // 001 101
    b.c[4] = *(const float*)(tabc + (b01 + z0)); b.c[5] = *(const float*)(tabc + (b11 + z0));      // 010 110
    b.c[6] = *(const float*)(tabc + (b01 + z1)); b.c[7] = *(const float*)(tabc + (b11 + z1));      // 011 111
    if (a.pr >= 0 && q < 3) {
      const float* __restrict__ Ap = A + (size_t)a.pr * 12 + 3 * q;
      const float* __restrict__ Pp = P + (size_t)a.pr * 12 + 3 * q;
      b.A[0] = Ap[0]; b.A[1] = Ap[1]; b.A[2] = Ap[2]; b.P[0] = Pp[0]; b.P[1] = Pp[1]; b.P[2] = Pp[2];
    }
    b.s = sample_of_node[k];
    if (b.s >= 0) { b.ap = a_pos[4 * ((size_t)b.s * B + r) + q]; b.ad = a_dir[4 * ((size_t)b.s * B + r) + q]; }
  };
  auto node = [&](int k, const AdjNodeA& a, const AdjNodeB& b) {
    const float rd = q < 3 ? a.rdn : 0.f;
    const float n = quad_bcast<3>(a.rdn);
    // position gradient of this lane's channel of the trilinear interpolant (trilinear_grad_finish, one channel): D[ax] = d c / d p_ax
    const float xd = quad_bcast<0>(b.t), yd = quad_bcast<1>(b.t), zd = quad_bcast<2>(b.t);
    const float ox = 1.0f - xd, oy = 1.0f - yd, oz = 1.0f - zd;
    const float d000 = b.c[0], d100 = b.c[1], d001 = b.c[2], d101 = b.c[3], d010 = b.c[4], d110 = b.c[5], d011 = b.c[6], d111 = b.c[7];
    auto lerp = [](float u, float v, float wu, float wv) { return u * wu + v * wv; };
    float D[3];
    D[0] = lerp(lerp(d100 - d000, d110 - d010, oy, yd), lerp(d101 - d001, d111 - d011, oy, yd), oz, zd) * rnx;
    D[1] = lerp(lerp(d010 - d000, d110 - d100, ox, xd), lerp(d011 - d001, d111 - d101, ox, xd), oz, zd) * rny;
    D[2] = lerp(lerp(d001 - d000, d101 - d100, ox, xd), lerp(d011 - d010, d111 - d110, ox, xd), oy, yd) * rnz;
    // dn / d p_q from lane 3 (channel 0 = n)
    const float n0 = quad_bcast<3>(D[0]), n1 = quad_bcast<3>(D[1]), n2 = quad_bcast<3>(D[2]);
    const float dn = q == 0 ? n0 : (q == 1 ? n1 : n2);
    const bool pair = a.pr >= 0;
    const float Am[3] = {pair ? b.A[0] : D[0], pair ? b.A[1] : D[1], pair ? b.A[2] : D[2]};      // row q of d grad / d rp (lanes 0..2)
    // column sums over the rows held by lanes 0..2, delivered to the lane of that column
    auto tvec = [&](const float (&row)[3], float x) {
      const float c0 = sum3(row[0] * x), c1 = sum3(row[1] * x), c2 = sum3(row[2] * x);
      return q == 0 ? c0 : (q == 1 ? c1 : c2);
    };
    if (pair) {
      const float Pm[3] = {b.P[0], b.P[1], b.P[2]};
      const float v = tvec(Pm, step * ld);                              // v = P^T (step lambda_d(k+1)): the cotangent of raw at this pair
      if (live) v_out[4 * (size_t)a.pr + q] = q < 3 ? v : 0.f;
    }
    const float s_n = step / n;
    const float rdlp = sum3(rd * lp);
    const float cfac = -s_n / n * rdlp;                               // c_k . = -step / n^2 * dn/dx * (rd . lambda_p)
    float nlp = lp + cfac * dn + step * tvec(Am, ld);
    float nld = ld + s_n * lp;
    if (b.s >= 0) {
      nlp += b.ap;
      // ray_dir = rd / sqrt(max(|rd|^2, 1e-6)) (safe_l2_normalize, eikonal_utils.py:113)
      const float q2 = sum3(rd * rd);
      if (q2 > 1e-6f) {
        const float inv = 1.0f / sqrtf(q2);
        const float u = rd * inv;
        const float au = sum3(b.ad * u);
        nld += (b.ad - au * u) * inv;
      } else {
        nld += b.ad * 1000.0f;                                        // 1 / sqrt(1e-6)
      }
    }
    lp = q < 3 ? nlp : 0.f; ld = q < 3 ? nld : 0.f;
  };
  // node k of trip position I: stage A of node k - 3 and stage B of node k - 2 are issued, then the arithmetic of node k runs (a node's
  // arithmetic is ~0.3 us, a round trip to the table about twice that: one node of lead was not enough).  4 A sets x 3 B sets.
  AdjNodeA xa[4];
  AdjNodeB yb[3];
  auto stage = [&](auto I, int k) {
    constexpr int i = decltype(I)::value;
    if (k >= 3) load_a(k - 3, xa[(i + 3) % 4]);
    if (k >= 2) load_b(k - 2, xa[(i + 2) % 4], yb[(i + 2) % 3]);
    node(k, xa[i % 4], yb[i % 3]);
  };
  int k = num_nodes - 1;
  load_a(k, xa[0]);
  if (k >= 1) load_a(k - 1, xa[1]);
  if (k >= 2) load_a(k - 2, xa[2]);
  load_b(k, xa[0], yb[0]);
  if (k >= 1) load_b(k - 1, xa[1], yb[1]);
#define RNERF_ADJ_STAGE(I) stage(std::integral_constant<int, I>(), k - I)
  for (; k >= 11; k -= 12) {
    RNERF_ADJ_STAGE(0); RNERF_ADJ_STAGE(1); RNERF_ADJ_STAGE(2); RNERF_ADJ_STAGE(3); RNERF_ADJ_STAGE(4); RNERF_ADJ_STAGE(5);
    RNERF_ADJ_STAGE(6); RNERF_ADJ_STAGE(7); RNERF_ADJ_STAGE(8); RNERF_ADJ_STAGE(9); RNERF_ADJ_STAGE(10); RNERF_ADJ_STAGE(11);
  }
  // the remaining 0 .. 11 nodes continue the same rotation
#define RNERF_ADJ_TAIL(I) if (k - I >= 0) RNERF_ADJ_STAGE(I)
  RNERF_ADJ_TAIL(0); RNERF_ADJ_TAIL(1); RNERF_ADJ_TAIL(2); RNERF_ADJ_TAIL(3); RNERF_ADJ_TAIL(4); RNERF_ADJ_TAIL(5);
  RNERF_ADJ_TAIL(6); RNERF_ADJ_TAIL(7); RNERF_ADJ_TAIL(8); RNERF_ADJ_TAIL(9); RNERF_ADJ_TAIL(10);
#undef RNERF_ADJ_TAIL
#undef RNERF_ADJ_STAGE
}

}  // namespace rnerf

using namespace rnerf;

extern "C" size_t rnerf_bkgd_save_bytes(int64_t n) { return bkgd_save_floats(n) * sizeof(float); }
extern "C" size_t rnerf_bkgd_dy_bytes(int64_t n) { return bkgd_dy_floats(n) * sizeof(float); }

extern "C" int rnerf_bkgd_backward(const float* params, const void* save, const float* d_out, int64_t n, double rgb_padding, void* dy,
                                   float* grads, float* d_dirs, void* stream) {
  RNERF_CHECK_ARG(params && save && d_out && dy && grads, "rnerf_bkgd_backward: null pointer");
  RNERF_CHECK_ARG(n >= 1, "rnerf_bkgd_backward: n must be >= 1");
  hipStream_t st = (hipStream_t)stream;
  const float* sv = (const float*)save;
  float* dyf = (float*)dy;
  hipLaunchKernelGGL(bkgd_dgrad_kernel, dim3((unsigned)((n + 31) / 32)), dim3(64), 0, st, params, sv, d_out, (long long)n, (float)(1 + 2 * rgb_padding),
                     (float)rgb_padding, dyf, (float4*)d_dirs);
  RNERF_CHECK_LAUNCH();
  const unsigned chunks = (unsigned)((n + 255) / 256);
  float* partial = dyf + (size_t)n * 5 * 128;
  hipLaunchKernelGGL(bkgd_wgrad_kernel<0>, dim3(((chunks + 7) / 8) * 8 * SmallNet<0>::UNITS), dim3(256), 0, st, sv, (const float*)dyf, (long long)n, partial);
  hipLaunchKernelGGL(bkgd_wgrad_reduce_kernel<RNERF_BKGDMLP_PARAMS>, dim3((RNERF_BKGDMLP_PARAMS + 255) / 256), dim3(256), 0, st, (const float*)partial, (int)chunks,
                     grads);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_so3_query(const float* table, const rnerf_grid* g, const float* so3_params, const float* window10, const float* pts,
                               const float* condition, int64_t n, float* out4, float* pred_grad, void* stream) {
  RNERF_CHECK_ARG(table && g && so3_params && window10 && pts && out4 && pred_grad, "rnerf_so3_query: null pointer");
  RNERF_CHECK_ARG(n >= 1, "rnerf_so3_query: n must be >= 1");
  GridParams gp;
  RNERF_CHECK_ARG(make_grid_params(g, &gp), "rnerf_so3_query: bad grid");
  So3Window w;
  for (int i = 0; i < 10; ++i) w.w[i] = window10[i];
  hipLaunchKernelGGL(so3_query_kernel, dim3((unsigned)((n + 31) / 32)), dim3(64), 0, (hipStream_t)stream, (const float4*)table, gp, so3_params, w,
                     pts, condition, (long long)n, (float4*)out4, pred_grad);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" size_t rnerf_so3_packed_bytes(void) { return (size_t)kSo3Blocks * 128 * sizeof(uint4); }

extern "C" int rnerf_march_all(const float* table, const rnerf_grid* g, const float* so3_params, void* so3_packed, const float* window10, const float* origins,
                               const float* viewdirs, int32_t B, double near, double far, int32_t num_nodes, float* path_pd, float* path_dr,
                               float* path_ior, const int32_t* ray_order, void* stream) {
  RNERF_CHECK_ARG(table && g && so3_params && so3_packed && window10 && origins && viewdirs && path_pd && path_dr, "rnerf_march_all: null pointer");
  RNERF_CHECK_ARG(B > 0 && num_nodes >= 2, "rnerf_march_all: need B > 0 and num_nodes >= 2");
  GridParams gp;
  RNERF_CHECK_ARG(make_grid_params(g, &gp), "rnerf_march_all: bad grid");
  So3Window w;
  for (int i = 0; i < 10; ++i) w.w[i] = window10[i];
  RNERF_CHECK_ARG(grid_fits_u32(gp), "rnerf_march_all: grid too large for 32-bit byte offsets (needs a table < 4 GiB and 24-bit strides of index >> 1: twice the row strides in reference order, the brick strides in bricks)");
  const float stepf = (float)((far - near) / (num_nodes - 1));  // models.py:122
  hipLaunchKernelGGL(so3_pack16_kernel, dim3((kSo3Blocks * 64 + 255) / 256), dim3(256), 0, (hipStream_t)stream, so3_params, (uint4*)so3_packed);
  hipLaunchKernelGGL(march_all_kernel, dim3((unsigned)((B + 15) / 16)), dim3(256), 0, (hipStream_t)stream, (const float4*)table, gp, so3_params,
                     (const uint4*)so3_packed, w, origins, viewdirs, B, (float)near, stepf, num_nodes, (float4*)path_pd, (float4*)path_dr, (float4*)path_ior,
                     (float4*)nullptr, (int*)nullptr, 0, (int2*)nullptr, (float4*)nullptr, (float4*)nullptr, (int*)nullptr, (const int*)ray_order);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_march_all_train(const float* table, const rnerf_grid* g, const float* so3_params, void* so3_packed, const float* window10, const float* origins,
                                     const float* viewdirs, int32_t B, double near, double far, int32_t num_nodes, float* path_pd, float* path_dr,
                                     float* path_rdn, int32_t* pair_count, int32_t pair_cap, int32_t* pair_id, float* pair_x, float* pair_g,
                                     int32_t* pair_of_node, const int32_t* ray_order, void* stream) {
  RNERF_CHECK_ARG(table && g && so3_params && so3_packed && window10 && origins && viewdirs && path_pd && path_dr && path_rdn && pair_count && pair_id && pair_x &&
                  pair_g && pair_of_node, "rnerf_march_all_train: null pointer");
  RNERF_CHECK_ARG(B > 0 && num_nodes >= 2 && pair_cap >= 1, "rnerf_march_all_train: need B > 0, num_nodes >= 2, pair_cap >= 1");
  GridParams gp;
  RNERF_CHECK_ARG(make_grid_params(g, &gp), "rnerf_march_all_train: bad grid");
  So3Window w;
  for (int i = 0; i < 10; ++i) w.w[i] = window10[i];
  RNERF_CHECK_ARG(grid_fits_u32(gp), "rnerf_march_all_train: grid too large for 32-bit byte offsets (needs a table < 4 GiB and 24-bit strides of index >> 1: twice the row strides in reference order, the brick strides in bricks)");
  const float stepf = (float)((far - near) / (num_nodes - 1));
  hipStream_t st = (hipStream_t)stream;
  RNERF_CHECK_HIP(hipMemsetAsync(pair_count, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(so3_pack16_kernel, dim3((kSo3Blocks * 64 + 255) / 256), dim3(256), 0, st, so3_params, (uint4*)so3_packed);
  hipLaunchKernelGGL(march_all_kernel, dim3((unsigned)((B + 15) / 16)), dim3(256), 0, st, (const float4*)table, gp, so3_params, (const uint4*)so3_packed, w, origins, viewdirs, B,
                     (float)near, stepf, num_nodes, (float4*)path_pd, (float4*)path_dr, (float4*)nullptr, (float4*)path_rdn, (int*)pair_count,
                     (int)pair_cap, (int2*)pair_id, (float4*)pair_x, (float4*)pair_g, (int*)pair_of_node, (const int*)ray_order);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" size_t rnerf_so3_save_bytes(int64_t n) { return so3_save_bytes_total(n); }
extern "C" size_t rnerf_so3_dy_bytes(int64_t nb) { return so3_dy_floats(nb) * sizeof(float); }

extern "C" int rnerf_so3_backward(const float* so3_params, const float* window10, const float* pts4, const void* save, int64_t n_save,
                                  const float* d_raw4, int64_t nb, void* dy, float* dx4, float* grads, void* stream) {
  RNERF_CHECK_ARG(so3_params && window10 && pts4 && save && d_raw4 && dy, "rnerf_so3_backward: null pointer");
  RNERF_CHECK_ARG(n_save >= 1 && nb >= 1, "rnerf_so3_backward: n_save, nb must be >= 1");
  RNERF_CHECK_ARG(!grads || nb == n_save, "rnerf_so3_backward: the parameter gradient needs one cotangent per saved row (nb == n_save)");
  So3Window w;
  for (int i = 0; i < 10; ++i) w.w[i] = window10[i];
  hipStream_t st = (hipStream_t)stream;
  float* dyf = (float*)dy;
  hipLaunchKernelGGL(so3_dgrad_kernel, dim3((unsigned)((nb + 31) / 32)), dim3(64), 0, st, so3_params, w, (const float4*)pts4, (const float*)save,
                     (long long)n_save, (const float4*)d_raw4, (long long)nb, grads ? dyf : (float*)nullptr, (float4*)dx4);
  if (grads) {
    const unsigned chunks = (unsigned)((nb + 256 * SmallNet<1>::CHUNKS_PER_WG - 1) / (256 * SmallNet<1>::CHUNKS_PER_WG));      // partials: one per workgroup
    float* partial = dyf + (size_t)nb * 5 * 128;
    hipLaunchKernelGGL(bkgd_wgrad_kernel<1>, dim3(((chunks + 7) / 8) * 8 * SmallNet<1>::UNITS), dim3(256), 0, st, (const float*)save, (const float*)dyf, (long long)nb, partial);
    hipLaunchKernelGGL(bkgd_wgrad_reduce_kernel<RNERF_SO3MLP_PARAMS>, dim3((RNERF_SO3MLP_PARAMS + 255) / 256), dim3(256), 0, st, (const float*)partial,
                       (int)chunks, grads);
  }
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_so3_pair_jacobian(const float* table, const rnerf_grid* g, const float* pair_x, const float* pair_g, const float* raw4,
                                       const float* J4, int64_t np, float* A12, float* P12, void* stream) {
  RNERF_CHECK_ARG(table && g && pair_x && pair_g && raw4 && J4 && A12 && P12, "rnerf_so3_pair_jacobian: null pointer");
  RNERF_CHECK_ARG(np >= 1, "rnerf_so3_pair_jacobian: np must be >= 1");
  GridParams gp;
  RNERF_CHECK_ARG(make_grid_params(g, &gp), "rnerf_so3_pair_jacobian: bad grid");
  hipLaunchKernelGGL(so3_pair_jacobian_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float4*)table, gp,
                     (const float4*)pair_x, (const float4*)pair_g, (const float4*)raw4, (const float4*)J4, (long long)np, A12, P12);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_march_adjoint(const float* table, const rnerf_grid* g, const float* path_pd, const float* path_rdn, const int32_t* pair_of_node,
                                   const float* A12, const float* P12, const float* a_pos, const float* a_dir, const int32_t* sample_of_node, int32_t B,
                                   double near, double far, int32_t num_nodes, float* v4, void* stream) {
  RNERF_CHECK_ARG(table && g && path_pd && path_rdn && pair_of_node && a_pos && a_dir && sample_of_node, "rnerf_march_adjoint: null pointer");
  RNERF_CHECK_ARG(B > 0 && num_nodes >= 2, "rnerf_march_adjoint: need B > 0 and num_nodes >= 2");
  GridParams gp;
  RNERF_CHECK_ARG(make_grid_params(g, &gp), "rnerf_march_adjoint: bad grid");
  RNERF_CHECK_ARG(grid_fits_u32(gp), "rnerf_march_adjoint: grid too large for 32-bit byte offsets (needs a table < 4 GiB and 24-bit strides of index >> 1: twice the row strides in reference order, the brick strides in bricks)");
  const float stepf = (float)((far - near) / (num_nodes - 1));
  hipLaunchKernelGGL(march_adjoint_kernel, dim3((unsigned)((B + 15) / 16)), dim3(64), 0, (hipStream_t)stream, (const float4*)table, gp,
                     (const float4*)path_pd, (const float4*)path_rdn, (const int*)pair_of_node, A12, P12, (const float4*)a_pos, (const float4*)a_dir,
                     (const int*)sample_of_node, B, num_nodes, stepf, (float4*)v4);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}
