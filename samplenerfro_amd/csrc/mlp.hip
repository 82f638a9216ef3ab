// Positional encoding + NerfMLP evaluation and training on the matrix cores (P1, N1).  The small MLPs (N2) are csrc/small_mlp.hip.
// Reference: rnerf/model_utils.py:187-214 (pos_enc), :30-90 (NerfMLP); call sites rnerf/models.py:257,289,
// 303-308,394,426,441.
//
// Design (gfx950, wave64, v_mfma_f32_32x32x16_{f16,bf16} / v_mfma_f32_32x32x2_f32):
//   * "Transposed chain": every layer is computed as  Y^T[n_out][row] = W^T[n_out][k] * X^T[k][row], i.e. the WEIGHTS are
//     the MFMA A operand and the 32 sample rows owned by a wave are the B operand / the lane index of the accumulator.
//     The C/D layout (lane = row, registers = output features) is then exactly a B-operand layout for the next layer: the
//     8 k-values a lane supplies per MFMA may be ANY 8 features as long as the A operand (pre-packed weights) uses the
//     same assignment, so activations never leave the register file between layers — no LDS round trip, no transpose,
//     no cross-lane exchange.  Lane (row m = lane&31, half h = lane>>5) holds features
//         n = 32*t + (r&3) + 8*(r>>2) + 4*h          (t = n-tile, r = accumulator register 0..15)
//     and feeds k-step s, slot j with feature 16*s + 8*(j>>2) + 4*h + (j&3)  (= accumulator (t=s>>1, r=8*(s&1)+j)).
//   * fp32 parity: the reference computes the MLP in fp32.  F16X3/BF16X3 split both operands into hi+lo 16-bit parts and
//     issue 3 MFMAs per tile (hi*hi + hi*lo + lo*hi, fp32 accumulate).  F16/BF16 issue one.
//   * A workgroup = 4 waves = 256 consecutive sample rows (64 per wave, two 32-row m-tiles); the weight stream (2.3 MB
//     for X3) is read from L2 through a double-buffered LDS ring with global_load_lds (16 B/lane), one slab = one k-step
//     of one layer, shared by the 4 waves: 1 KB of L2->LDS traffic per row and layer.
//   * Persistent grid: each workgroup walks row tiles with stride gridDim.x and prefetches across layer and tile seams.
#include "common.h"
#include "nerfmlp_layout.h"
#include "mfma_ops.h"

#include <stdlib.h>
#include <type_traits>
#include <vector>
#include <stdio.h>

namespace rnerf {


#define GLOBAL_AS __attribute__((address_space(1)))
#define LDS_AS __attribute__((address_space(3)))

// The 10 MFMA layers: Dense_0..Dense_7 (trunk), Dense_9 (bottleneck), Dense_10 (view layer).
// kind: 0 = input is the 63-d positional encoding; 1 = previous activations; 2 = previous + PE (skip concat,
// rnerf/model_utils.py:68-69); 3 = previous (bottleneck) + 27-d view encoding (:82-83).
struct MfmaLayer { int dense, ks, nt, kind; };
__host__ __device__ constexpr MfmaLayer mfma_layer(int l) {
  constexpr MfmaLayer t[10] = {{0, 4, 8, 0},  {1, 16, 8, 1}, {2, 16, 8, 1}, {3, 16, 8, 1}, {4, 16, 8, 1},
                               {5, 20, 8, 2}, {6, 16, 8, 1}, {7, 16, 8, 1}, {9, 16, 8, 1}, {10, 18, 4, 3}};
  return t[l];
}
__host__ __device__ constexpr int layer_blocks_before(int l) {   // in units of (kstep, ntile) 1-KiB-per-part blocks
  int o = 0;
  for (int i = 0; i < l; ++i) o += mfma_layer(i).ks * mfma_layer(i).nt;
  return o;
}
constexpr int kTotalBlocks = layer_blocks_before(10);   // 1160

// aux section (floats) that follows the weight stream: fp32 biases in natural feature order, sigma/rgb heads.
constexpr int AUX_BIAS = 0;            // 10 layers x 256
constexpr int AUX_WSIG = 2560;         // Dense_8 kernel [256]
constexpr int AUX_BSIG = 2816;         // Dense_8 bias (+3 pad)
constexpr int AUX_WRGB = 2820;         // Dense_11 kernel transposed [3][128]
constexpr int AUX_BRGB = 3204;         // Dense_11 bias (+1 pad)
constexpr int AUX_ZERO = 3208;         // 256 zeros: the sigma weights of every layer but the trunk output (PrevConv SIG)
constexpr int AUX_FLAG = 3464;         // f16 modes: non-zero = a weight left the f16 range of the scaled stream (|W| >= 256 for the 2^8-scaled streams: the
                                       // forward returns NaN, never a plausible wrong colour; |W| >= 3.99 for f16f8's 2^14: the launch falls back to f16x3)
constexpr int AUX_FLOATS = 3468;

template <int PREC>
struct Prec {
  static constexpr bool F16 = (PREC == RNERF_PREC_F16X3 || PREC == RNERF_PREC_F16 || PREC == RNERF_PREC_F16X2 || PREC == RNERF_PREC_F16F8);
  // F8X: f16 main term + the two cross terms of the hi/lo split on v_mfma_f32_32x32x16_fp8_fp8 (e4m3).  The cross terms carry 2^-11 of the
  // product and need 4 bits, not 11: same instruction count and operand bytes as f16x3, but the fp8 MFMA draws less power, and with every CU
  // busy the engine is power-limited (tools/ubench/mfma_fp8.hip: 16.8 instead of 19.4 ns per MFMA for a 1 f16 + 2 fp8 mix).  Second block of a
  // weight tile = [fp8(W_lo) x 8 | fp8(W 2^-10) x 8] per lane, second operand part = [fp8(x) x 8 | fp8(x_lo 2^10) x 8]: with the weights
  // scaled by 2^14 both factors of both terms sit in the middle of e4m3's range without any block scale (W_lo ~ 4 W, x_lo 2^10 ~ x / 4).
  static constexpr bool F8X = PREC == RNERF_PREC_F16F8;
  static constexpr int NP = (PREC == RNERF_PREC_F16X3 || PREC == RNERF_PREC_BF16X3 || PREC == RNERF_PREC_F16X2 || F8X) ? 2 : 1;   // parts of a WEIGHT
  // MFMA passes per tile of a two-part stream: 3 = W_hi x_hi + W_lo x_hi + W_hi x_lo (fp32-grade);
  // 22 = (W_hi + W_lo) x_hi (f16x2: exact weights, activations rounded to f16 — 2/3 of the matrix work)
  // 38 = W_hi x_hi (f16) + W_lo x (fp8) + W x_lo (fp8)
  static constexpr int PASSES = PREC == RNERF_PREC_F16X2 ? 22 : (F8X ? 38 : 3);
  // power-of-two weight scale: keeps the lo part of an f16 split out of the f16 subnormal range (f16f8: |W| must stay below 3.99)
  static constexpr float WSCALE = F8X ? 16384.f : (F16 ? 256.f : 1.f);
  static constexpr size_t STREAM_BYTES = (size_t)kTotalBlocks * NP * 1024;
  static constexpr int SLAB = 8 * NP * 1024;        // one slab = 1 k-step of an N=256 layer = 2 k-steps of the N=128 view layer
  static constexpr size_t PACKED_BYTES = STREAM_BYTES + (size_t)AUX_FLOATS * 4;
};

// ---- fp8 (e4m3) cross-term operands of the f16f8 precision ------------------------------------------------------------------
constexpr float F8X_LO_SCALE = 1024.f;       // x_lo is multiplied, the W image of the second cross term divided by it
// two values -> two fp8 bytes in half `HI` of `old` (the other half is kept).  Written as the instruction: the LOW half is a plain output
// (the builtin takes the old value as an input, and an "old" that does not exist yet is an undefined register the allocator spills and
// reloads); SCALED = v_cvt_scalef32_pk_fp8_f32, which divides by its scale operand (the power of two 1 / F8X_LO_SCALE).  Overflow: with
// MODE.FP16_OVFL set (f8x_mode()) the conversion clamps to +-448, without it a value above ~464 becomes NaN (probed: fp8_cvt_probe.hip).
// ORDER CONTRACT: the LOW half of a word must be converted BEFORE its HIGH half (the LOW form starts a fresh register and would drop a high
// half written earlier).  Every caller walks the value pairs p = 0, 1, 2, 3 upwards (f8x_lo_part, PrevConv / EncWork chunks, the pack
// kernel); f8_word() below builds a whole word in the right order for new callers.
template <bool HI, bool SCALED = false>
__device__ __forceinline__ uint32_t f8_pair(uint32_t old, float a, float b) {
  uint32_t r = old;
  const float inv = 1.0f / F8X_LO_SCALE;
  if constexpr (!SCALED) {
    if constexpr (HI) asm("v_cvt_pk_fp8_f32 %0, %1, %2 op_sel:[0,0,1]" : "+v"(r) : "v"(a), "v"(b));
    else asm("v_cvt_pk_fp8_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  } else {
    if constexpr (HI) asm("v_cvt_scalef32_pk_fp8_f32 %0, %1, %2, %3 op_sel:[0,0,0,1]" : "+v"(r) : "v"(a), "v"(b), "v"(inv));
    else asm("v_cvt_scalef32_pk_fp8_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(inv));
  }
  return r;
}
// one whole fp8 word from four values, low half first (the order contract of f8_pair in one place)
template <bool SCALED = false>
__device__ __forceinline__ uint32_t f8_word(float a, float b, float c, float d) {
  return f8_pair<true, SCALED>(f8_pair<false, SCALED>(0u, a, b), c, d);
}
// fp8 conversions clamp instead of producing NaN: MODE.FP16_OVFL (bit 23); set once at the head of an f16f8 kernel
__device__ __forceinline__ void f8x_mode() { asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 1"); }
__device__ __forceinline__ f32x16 mfma_f8(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, const f32x16 c) {
  const long A = (long)(((unsigned long long)a1 << 32) | a0), B = (long)(((unsigned long long)b1 << 32) | b0);
  return __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(A, B, c, 0, 0, 0);
}
// lo part of an operand in the f16f8 layout from 8 values and their f16 hi parts: [fp8(x) x 8 | fp8((x - hi) 2^10) x 8]
__device__ __forceinline__ uint4 f8x_lo_part(const float (&x)[8], const uint32_t (&h)[4]) {
  uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    float ha, hb;
    unpack2<true>(h[p], ha, hb);
    const float r0 = x[2 * p] - ha, r1 = x[2 * p + 1] - hb;
    if (p & 1) { o[p >> 1] = f8_pair<true>(o[p >> 1], x[2 * p], x[2 * p + 1]); o[2 + (p >> 1)] = f8_pair<true, true>(o[2 + (p >> 1)], r0, r1); }
    else { o[p >> 1] = f8_pair<false>(o[p >> 1], x[2 * p], x[2 * p + 1]); o[2 + (p >> 1)] = f8_pair<false, true>(o[2 + (p >> 1)], r0, r1); }
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

// ---- 8-bit lo planes of the training tensors (backward mode RNERF_BWD_F16X3_LO8) ------------------------------------------------------
// The lo part of an operand (x - f16(x): at most half an ulp of the hi part) is STORED as e4m3 of lo / scale and decoded back to f16 by the
// wgrad (v_cvt_scalef32_pk_f16_fp8 multiplies by the same scale operand; probed: tools/ubench/tr8_cvt_probe.hip): hi 2 B + lo 1 B per
// value.  Fixed power-of-two scales: saved activations 2^-13 (full 3-bit lo significand for 0.004 <= |x| < 128, absolute resolution
// 2^-22 below, the lo part clamped — f16-hi precision — above), gradients 2^-14 (rows are normalised to 32 <= max |d raw| < 64: full
// precision for 2^-7 <= |dY| < 64).  Overflow: v_cvt_scalef32_pk_fp8_f16 returns NaN above 448 unless MODE.FP16_OVFL is set — the training
// forward sets it (its range watch then takes f16's clamp value as "left the range", like f16f8), the dgrad clamps the f16 lo parts first
// (its f16 overflow must stay inf: that is how a gradient chain that left its headroom shows).
constexpr float LO8_SCALE_X = 1.0f / 8192.f, LO8_SCALE_D = 1.0f / 16384.f;
template <bool HI>
__device__ __forceinline__ uint32_t lo8_pair(uint32_t old, uint32_t f16x2, float scale) {      // ORDER CONTRACT of f8_pair: low half first
  uint32_t r = old;
  if constexpr (HI) asm("v_cvt_scalef32_pk_fp8_f16 %0, %1, %2 op_sel:[0,0,1]" : "+v"(r) : "v"(f16x2), "v"(scale));
  else asm("v_cvt_scalef32_pk_fp8_f16 %0, %1, %2" : "=v"(r) : "v"(f16x2), "v"(scale));
  return r;
}
template <bool CLAMP>
__device__ __forceinline__ uint2 lo8_pack(const uint4& lo, float scale) {
  uint32_t w[4] = {lo.x, lo.y, lo.z, lo.w};
  if constexpr (CLAMP) {      // |lo| <= 448 scale as packed f16 (448 * 2^-14 = 0.02734375 = 0x2700)
    static_assert(LO8_SCALE_D == 1.0f / 16384.f, "clamp constant");
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      asm("v_pk_min_f16 %0, %0, %1" : "+v"(w[p]) : "v"(0x27002700u));
      asm("v_pk_max_f16 %0, %0, %1" : "+v"(w[p]) : "v"(0xA700A700u));
    }
  }
  uint2 o;
  o.x = lo8_pair<true>(lo8_pair<false>(0u, w[0], scale), w[1], scale);
  o.y = lo8_pair<true>(lo8_pair<false>(0u, w[2], scale), w[3], scale);
  return o;
}
typedef int int2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ half8 lo8_decode(const int2v v, float scale) {      // 8 e4m3 bytes -> 8 f16 (x scale)
  const half2v a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((unsigned)v.x, scale, false), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((unsigned)v.x, scale, true);
  const half2v c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((unsigned)v.y, scale, false), d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((unsigned)v.y, scale, true);
  return half8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}


// input feature (row of the Dense kernel) for MFMA layer l, k-step s, half h, slot j; -1 = zero padding
__host__ __device__ constexpr int in_feature(int l, int s, int h, int j) {
  const int kind = mfma_layer(l).kind;
  if (kind == 0) return pe_feature(8 * s + j, h);
  if (s < 16) return prev_feature(s, h, j);
  if (kind == 2) { const int f = pe_feature(8 * (s - 16) + j, h); return f < 0 ? -1 : 256 + f; }
  const int f = view_feature(8 * (s - 16) + j, h);
  return f < 0 ? -1 : 256 + f;
}

// ---- pack kernel: flat fp32 params -> MFMA A-operand stream + aux ---------------------------------------------------------
template <int PREC>
__global__ void nerfmlp_pack_kernel(const float* __restrict__ params, char* __restrict__ packed) {
  using PP = Prec<PREC>;
  constexpr bool F16 = PP::F16;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;   // one thread per (block, lane): 8 slots
  if (gid < kTotalBlocks * 64) {
    const int blk = gid >> 6, lane = gid & 63;
    int l = 0;
    while (l < 9 && blk >= layer_blocks_before(l + 1)) ++l;
    const int rel = blk - layer_blocks_before(l);
    const int nt = mfma_layer(l).nt, s = rel / nt, t = rel % nt;
    const int d = mfma_layer(l).dense, out_dim = nerf_dense(d).out;
    const int n_out = 32 * t + (lane & 31), h = lane >> 5;
    float w[8];
    for (int j = 0; j < 8; ++j) {
      const int f = in_feature(l, s, h, j);
      w[j] = f < 0 ? 0.f : params[nerf_koff(d) + f * out_dim + n_out] * PP::WSCALE;
      if constexpr (PP::F16) { if (!(fabsf(w[j]) <= 65504.f)) ((float*)(packed + PP::STREAM_BYTES))[AUX_FLAG] = 1.0f; }   // zeroed by the launcher
    }
    uint32_t hi[4], lo[4];
    for (int p = 0; p < 4; ++p) split2<F16>(w[2 * p], w[2 * p + 1], hi[p], lo[p]);
    if constexpr (PP::F8X) {      // [fp8(W_lo) x 8 | fp8(W / 2^10) x 8]
      f8x_mode();
      float wl[8], ws[8];
      for (int p = 0; p < 4; ++p) {
        float ha, hb;
        unpack2<true>(hi[p], ha, hb);
        wl[2 * p] = w[2 * p] - ha; wl[2 * p + 1] = w[2 * p + 1] - hb;
        ws[2 * p] = w[2 * p] * (1.0f / F8X_LO_SCALE); ws[2 * p + 1] = w[2 * p + 1] * (1.0f / F8X_LO_SCALE);
      }
      lo[0] = f8_pair<true>(f8_pair<false>(0u, wl[0], wl[1]), wl[2], wl[3]); lo[1] = f8_pair<true>(f8_pair<false>(0u, wl[4], wl[5]), wl[6], wl[7]);
      lo[2] = f8_pair<true>(f8_pair<false>(0u, ws[0], ws[1]), ws[2], ws[3]); lo[3] = f8_pair<true>(f8_pair<false>(0u, ws[4], ws[5]), ws[6], ws[7]);
    }
    uint4* dst = (uint4*)(packed + (size_t)blk * PP::NP * 1024);
    dst[lane] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    if constexpr (PP::F8X) { uint2* d2 = (uint2*)(dst + 64); d2[lane] = make_uint2(lo[0], lo[1]); d2[64 + lane] = make_uint2(lo[2], lo[3]); }
    else if (PP::NP == 2) dst[64 + lane] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
  }
  float* aux = (float*)(packed + PP::STREAM_BYTES);
  if (gid < AUX_FLAG) {
    float v = 0.f;
    if (gid < AUX_WSIG) {
      const int l = gid >> 8, n = gid & 255, d = mfma_layer(l).dense;
      v = n < nerf_dense(d).out ? params[nerf_boff(d) + n] : 0.f;
    } else if (gid < AUX_BSIG) v = params[nerf_koff(8) + (gid - AUX_WSIG)];
    else if (gid == AUX_BSIG) v = params[nerf_boff(8)];
    else if (gid >= AUX_WRGB && gid < AUX_BRGB) { const int c = (gid - AUX_WRGB) / 128, n = (gid - AUX_WRGB) % 128; v = params[nerf_koff(11) + n * 3 + c]; }
    else if (gid >= AUX_BRGB && gid < AUX_BRGB + 3) v = params[nerf_boff(11) + (gid - AUX_BRGB)];
    aux[gid] = v;
  }
}

// ---- forward kernel -----------------------------------------------------------------------------------------------------
// Weight-stream DMA (global -> LDS, 16 B per lane, 1 KiB per wave-instruction).  Written as inline asm on purpose: for the
// __builtin_amdgcn_global_load_lds form hipcc orders every later ds_read behind the DMA (it cannot prove the reads hit the
// OTHER ring slot) and emits s_waitcnt vmcnt(0) right after the issue, which serialises the prefetch with the compute.
// The asm form is invisible to the compiler's counters; slab_wait_dma() before the slab-end barrier is the only wait.
// lds_off: wave-uniform LDS byte address (dynamic LDS starts at 0: the kernel has no static __shared__).
__device__ __forceinline__ void glds16(const char* gsrc, unsigned lds_off) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_off) : "memory");
}
// the same with the non-temporal policy: operand streams that are read exactly once (wgrad)
__device__ __forceinline__ void glds16_nt(const char* gsrc, unsigned lds_off) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_off) : "memory");
}
// the same with a wave-uniform 64-bit base (SGPR pair) + a 32-bit per-lane byte offset: the address arithmetic of a stream that advances
// by a uniform stride runs on the scalar unit and the lane part costs one VGPR instead of two
__device__ __forceinline__ void glds16_nt_s(const char* sbase, unsigned voff, unsigned lds_off) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_off) : "memory");
}
// vmcnt(0) as the BUILTIN (imm: vmcnt=0, expcnt=7, lgkmcnt=15): hipcc folds an explicit s_waitcnt into its own scoreboard,
// so it also knows that every load it tracks itself (bias prefetch) has landed and emits no stricter wait later.
__device__ __forceinline__ void slab_wait_dma() { __builtin_amdgcn_s_waitcnt(0x0F70); asm volatile("" ::: "memory"); }

template <int BYTES>
__device__ __forceinline__ void issue_slab(const char* __restrict__ gsrc, unsigned lds_off, int wave, int lane) {
  constexpr int PER_WAVE = BYTES / 4;
  constexpr int N = PER_WAVE / 1024;
  static_assert(N >= 1 && N * 4096 == BYTES, "slab must be a multiple of 4 KiB");
#pragma unroll
  for (int c = 0; c < N; ++c)
    glds16(gsrc + wave * PER_WAVE + c * 1024 + lane * 16,
           __builtin_amdgcn_readfirstlane(lds_off + wave * PER_WAVE + c * 1024));   // hardware adds lane*16
}

// B operands of one k-step for the wave's two 32-row m-tiles
// min(u16, 1) of both halves of a dword = the non-zero flags of two non-negative 16-bit floats.  Written as the instruction:
// hipcc expands __builtin_elementwise_min(u16x2, {1,1}) into ~20 SDWA compares / scalar mask ops per dword.
__device__ __forceinline__ uint32_t pk_maxu(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_pk_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ uint32_t pk_min1(uint32_t w) {
  uint32_t r;
  asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(w), "v"(0x00010001u));
  return r;
}

// 16-byte load through an explicitly GLOBAL pointer (a pointer that went through an asm operand is generic to hipcc: flat_load + 64-bit
// address arithmetic per load)
typedef float f32x4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 gload4(const float* p) {
  const f32x4v v = *(const __attribute__((address_space(1))) f32x4v*)p;
  return make_float4(v.x, v.y, v.z, v.w);
}

// B operands of one k-step for the two 32-row m-tiles of a wave.  ONE: the wave runs a single m-tile (128-row workgroup tiles for launches
// that would leave more than half of the CUs without a 256-row tile): everything of m-tile 1 — MFMAs, conversions, LDS state, saves — is
// compiled out; h1 / l1 are never read.
template <bool ONE_> struct KOpsT { static constexpr bool ONE = ONE_; uint4 h0, l0, h1, l1; };
typedef KOpsT<false> KOps;

// ReLU as an INTEGER max on the bit pattern: max_i32(bits(x), 0) is x for x >= +0, +0 for every negative x (and -0), and — unlike
// v_max_f32, which returns the non-NaN operand — it keeps +inf and NaN.  That matters because the activations travel as f16 parts: a hidden
// activation above 65504 becomes hi = inf, lo = x - inf = -inf, the next layer's sums inf - inf = NaN, and with fmaxf(NaN, 0) = 0 every unit
// of that layer silently read 0 — finite, plausible, wrong outputs (found in round 4; DESIGN.md section 3.2, "Range").  With the integer max the NaN
// reaches the outputs: out of range means non-finite, never plausible.  NO_FLOOR (= INT_MIN) turns the max into the identity (bottleneck).
constexpr int RELU_FLOOR = 0, NO_FLOOR = (int)0x80000000u;
__device__ __forceinline__ float relu_keep(float x, int floor_bits) {
  const int b = __builtin_bit_cast(int, x);
  return __builtin_bit_cast(float, b > floor_bits ? b : floor_bits);
}

// streaming accesses of the training tensors (written once, read once by a later kernel): keep them out of the L2 working set
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void stream_store(uint4* p, const uint4 v) {
  u32x4_t t = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(t, (u32x4_t*)p);
}
__device__ __forceinline__ uint4 stream_load(const uint4* p) {
  const u32x4_t t = __builtin_nontemporal_load((const u32x4_t*)p);
  return make_uint4(t.x, t.y, t.z, t.w);
}
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void stream_store8(uint2* p, const uint2 v) {
  u32x2_t t = {v.x, v.y};
  __builtin_nontemporal_store(t, (u32x2_t*)p);
}

template <int PREC>
__device__ __forceinline__ void split8(const float (&x)[8], uint4& hi, uint4& lo) {
  using PP = Prec<PREC>;
  uint32_t h[4], l[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if constexpr (PP::NP == 2 && !PP::F8X) split2<PP::F16>(x[2 * p], x[2 * p + 1], h[p], l[p]);
    else { h[p] = pack2<PP::F16>(x[2 * p], x[2 * p + 1]); l[p] = 0; }
  }
  hi = make_uint4(h[0], h[1], h[2], h[3]);
  if constexpr (PP::F8X) lo = f8x_lo_part(x, h);
  else lo = make_uint4(l[0], l[1], l[2], l[3]);
}

// Conversion of the previous layer's outputs into the B operands of the NEXT k-step, cut into small chunks that are issued
// between the MFMAs of the CURRENT k-step (each MFMA occupies the matrix pipe for 32 cycles; an in-order wave can issue
// ~5 independent VALU ops in that shadow).  hipcc does not build this interleave by itself (it emits the ~110 VALU ops as
// one clump ahead of the 48 MFMAs and the matrix pipe idles), so the order is written out and pinned with sched_barrier.
//   pair pi in [0,8): m-tile pi>>2, value pair pi&3 -> chunk 0: bias+scale+ReLU, chunk 1: hi + residual, chunk 2: lo
// SIG: also accumulate sg0/sg1 += x * ws[j] (the sigma head, Dense_8, rides on the conversion of the trunk output that feeds Dense_9: the
// same relu(acc / scale + b) values; for every other layer ws points at zeros — no branch in the shared loop body).
template <int PREC, int S, bool MASK = false, bool SIG = false, bool ONE = false>
struct PrevConv {
  using PP = Prec<PREC>;
  float ws[8];
  float sg0 = 0.f, sg1 = 0.f;
  uint32_t nz[2] = {0, 0};   // MASK (training forward): non-zero flags of the 8 hi values per m-tile, bits p and 16 + p for pair p
  const f32x16& p0;   // m-tile 0: the accumulator registers holding features 32*(S>>1) .. +31 of the previous layer
  float v1[8];        // m-tile 1: raw accumulator values of the 8 features of k-step S (from LDS)
  float b[8];         // fp32 bias of the producing layer
  __device__ __forceinline__ PrevConv(const f32x16& p) : p0(p) {}
  int floor_v;     // RELU_FLOOR (ReLU) or NO_FLOOR (bottleneck: no activation) — see relu_keep()
  uint32_t hi[2][4], lo[2][4];
  // the pair in flight, per m-tile (a 4-tile k-step runs one pair of each m-tile at a time: PairOfPairs).  Four scalars, not arrays:
  // the inline asm below takes them by "+v", and an array member whose element goes into an asm operand stays in memory (scratch)
  float x0m0, x1m0, x0m1, x1m1;

  // five dependent stages of one value pair, one stage per MFMA slot (each stage = 1-2 independent VALU ops)
  template <int C, int PI>
  __device__ __forceinline__ void chunk() {
    constexpr int mt = PI >> 2, p = PI & 3;
    if constexpr (ONE && mt == 1) return;
    constexpr float INV_SCALE = 1.0f / PP::WSCALE;
    float& x0 = mt == 0 ? x0m0 : x0m1;
    float& x1 = mt == 0 ? x1m0 : x1m1;
    if constexpr (C == 0) {
      const float r0 = mt == 0 ? p0[8 * (S & 1) + 2 * p] : v1[2 * p];
      const float r1 = mt == 0 ? p0[8 * (S & 1) + 2 * p + 1] : v1[2 * p + 1];
      x0 = fmaf(r0, INV_SCALE, b[2 * p]);
      x1 = fmaf(r1, INV_SCALE, b[2 * p + 1]);
    } else if constexpr (C == 1) {
      x0 = relu_keep(x0, floor_v);
      x1 = relu_keep(x1, floor_v);
      if constexpr (SIG) {
        // volatile asm: as plain fmaf() the two FMAs are sunk below the residual stage (which overwrites x0 / x1 in place), and the
        // copies of x0 / x1 that keeps alive are spilled — 16 scratch stores per k-step
        float& sg = mt == 0 ? sg0 : sg1;
        asm volatile("v_fmac_f32_e32 %0, %1, %2" : "+v"(sg) : "v"(x0), "v"(ws[2 * p]));
        asm volatile("v_fmac_f32_e32 %0, %1, %2" : "+v"(sg) : "v"(x1), "v"(ws[2 * p + 1]));
      }
    } else if constexpr (C == 2) {
      hi[mt][p] = pack2<PP::F16>(x0, x1);
      if constexpr (PP::F8X) lo[mt][p >> 1] = f8_pair<(p & 1) != 0>(lo[mt][p >> 1], x0, x1);       // fp8(x): the operand of the W_lo term
    } else if constexpr (C == 3) {
      if constexpr (PP::NP == 2) {
        if constexpr (PP::F16) {   // x - (float)hi as one v_fma_mix_f32 per value (exact: the residual is representable)
          // written as the instruction: hipcc lowers fmaf((float)half, -1, x) to v_cvt_f32_f16 + v_add_f32 (2 ops per value)
          const uint32_t hw = hi[mt][p];
          asm("v_fma_mix_f32 %0, %1, -1.0, %0 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "+v"(x0) : "v"(hw));
          asm("v_fma_mix_f32 %0, %1, -1.0, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(x1) : "v"(hw));
        } else {
          float ha, hb;
          unpack2<false>(hi[mt][p], ha, hb);
          x0 -= ha; x1 -= hb;
        }
      }
    } else {
      if constexpr (PP::F8X) lo[mt][2 + (p >> 1)] = f8_pair<(p & 1) != 0, true>(lo[mt][2 + (p >> 1)], x0, x1);   // fp8(x_lo 2^10)
      else if constexpr (PP::NP == 2) lo[mt][p] = pack2<PP::F16>(x0, x1);
      else lo[mt][p] = 0;
      if constexpr (MASK) nz[mt] |= pk_min1(hi[mt][p]) << p;   // post-ReLU values are non-negative: min(u16, 1) = non-zero flag of each half
    }
  }
  __device__ __forceinline__ KOpsT<ONE> result() const {
    KOpsT<ONE> o;
    o.h0 = make_uint4(hi[0][0], hi[0][1], hi[0][2], hi[0][3]); o.l0 = make_uint4(lo[0][0], lo[0][1], lo[0][2], lo[0][3]);
    if constexpr (ONE) { o.h1 = o.h0; o.l1 = o.l0; }
    else { o.h1 = make_uint4(hi[1][0], hi[1][1], hi[1][2], hi[1][3]); o.l1 = make_uint4(lo[1][0], lo[1][1], lo[1][2], lo[1][3]); }
    return o;
  }
};

struct NoWork {
  template <int C, int PI>
  __device__ __forceinline__ void chunk() {}
};
// a k-step of 4 tiles (the view layer's N = 128) has half the MFMA slots: tile T carries pair T of BOTH m-tiles
template <typename W>
struct PairOfPairs {
  W& w;
  __device__ __forceinline__ PairOfPairs(W& w_) : w(w_) {}
  template <int C, int PI>
  __device__ __forceinline__ void chunk() {
    if constexpr (PI < 4) { w.template chunk<C, PI>(); w.template chunk<C, PI + 4>(); }
  }
};

// Position-encoding operands of k-step S (slot map pe_feature: slot q = 8 S + j < NSIN is sin(2^(q/3) x_(q%3) + phase(h)), then the
// identity terms) for both m-tiles, one value pair per MFMA tile like PrevConv: stage 0 argument + reduction index, 1 reduced argument,
// 2 sine polynomial, 3 cosine polynomial + selection, 4 hi / lo split.  Same arithmetic, same order as enc_ops() / pe_sin().
template <int PREC, int S, int NSIN, bool ONE = false>
struct EncWork {
  using PP = Prec<PREC>;
  const float4 (&v)[2];
  const int h;
  uint32_t hi[2][4], lo[2][4];
  PeSin e0, e1;
  float f0, f1;
  __device__ __forceinline__ EncWork(const float4 (&v_)[2], int h_) : v(v_), h(h_) {}
  template <int MT, int Q>
  __device__ __forceinline__ float coord() const {      // x, y or z of m-tile MT for sine slot Q
    constexpr int c = Q % 3;
    return c == 0 ? v[MT].x : (c == 1 ? v[MT].y : v[MT].z);
  }
  template <int MT, int Q>
  __device__ __forceinline__ float plain() const {      // the non-sine slots
    if constexpr (Q == NSIN) return h ? v[MT].z : v[MT].x;
    else if constexpr (Q == NSIN + 1) return h ? 0.f : v[MT].y;
    else return 0.f;
  }
  template <int C, int PI>
  __device__ __forceinline__ void chunk() {
    constexpr int mt = PI >> 2, p = PI & 3, q0 = 8 * S + 2 * p, q1 = q0 + 1;
    if constexpr (ONE && mt == 1) return;
    const float phase = h ? 1.5707963705062866f : 0.0f;   // f32(0.5*pi) (rnerf/model_utils.py:213)
    if constexpr (C == 0) {
      if constexpr (q0 < NSIN) e0.s0(fadd(fmul(coord<mt, q0>(), (float)(1 << (q0 / 3))), phase));
      if constexpr (q1 < NSIN) e1.s0(fadd(fmul(coord<mt, q1>(), (float)(1 << (q1 / 3))), phase));
    } else if constexpr (C == 1) {
      if constexpr (q0 < NSIN) e0.s1();
      if constexpr (q1 < NSIN) e1.s1();
    } else if constexpr (C == 2) {
      if constexpr (q0 < NSIN) e0.s2();
      if constexpr (q1 < NSIN) e1.s2();
    } else if constexpr (C == 3) {
      if constexpr (q0 < NSIN) f0 = e0.s3(); else f0 = plain<mt, q0>();
      if constexpr (q1 < NSIN) f1 = e1.s3(); else f1 = plain<mt, q1>();
    } else {
      if constexpr (PP::F8X) {
        hi[mt][p] = pack2<true>(f0, f1);
        float ha, hb;
        unpack2<true>(hi[mt][p], ha, hb);
        lo[mt][p >> 1] = f8_pair<(p & 1) != 0>(lo[mt][p >> 1], f0, f1);
        lo[mt][2 + (p >> 1)] = f8_pair<(p & 1) != 0, true>(lo[mt][2 + (p >> 1)], f0 - ha, f1 - hb);
      } else if constexpr (PP::NP == 2) split2<PP::F16>(f0, f1, hi[mt][p], lo[mt][p]);
      else { hi[mt][p] = pack2<PP::F16>(f0, f1); lo[mt][p] = 0; }
    }
  }
  __device__ __forceinline__ KOpsT<ONE> result() const {
    KOpsT<ONE> o;
    o.h0 = make_uint4(hi[0][0], hi[0][1], hi[0][2], hi[0][3]); o.l0 = make_uint4(lo[0][0], lo[0][1], lo[0][2], lo[0][3]);
    if constexpr (ONE) { o.h1 = o.h0; o.l1 = o.l0; }
    else { o.h1 = make_uint4(hi[1][0], hi[1][1], hi[1][2], hi[1][3]); o.l1 = make_uint4(lo[1][0], lo[1][1], lo[1][2], lo[1][3]); }
    return o;
  }
};

// Work of the LAST k-step of a layer (the layer seam), in the shadow of its MFMAs: once the MFMAs of tile t have been issued, tile
// t - 1 is final, so in tile t's slots
//   * its m-tile 0 outputs move to prev0[t - 1], its m-tile 1 outputs to the wave's LDS state (128 register moves + 32 ds_write_b128
//     per wave, which used to run after the k-step with the matrix pipe idle), and
//   * the operands of the NEXT layer's k-step 0 (features 0..15 = tile 0, registers 0..7) are converted from the final accumulators
//     (used to be prev_ops(0) at the head of the next layer, exposed together with its bias load).
// Tile 7 is handed over by finish() after the k-step.
template <int PREC, bool MASK, bool ONE = false>
struct SeamWork {
  f32x16 (&acc0)[8];
  f32x16 (&acc1)[8];
  f32x16 (&prev0)[8];
  float4* st1;
  PrevConv<PREC, 0, MASK, true, ONE> cv;      // pairs 0..3: m-tile 0 from acc0[0], pairs 4..7: m-tile 1 from acc1[0]
  __device__ __forceinline__ SeamWork(f32x16 (&a0)[8], f32x16 (&a1)[8], f32x16 (&p0)[8], float4* s1) : acc0(a0), acc1(a1), prev0(p0), st1(s1), cv(a0[0]) {}
  template <int C, int T>
  __device__ __forceinline__ void move() {            // piece C of the hand-over of tile T
    // (the m-tile 0 moves are plain assignments: hipcc sinks them to the head of the next layer, ~1 k clocks per layer; pinning them here
    // with volatile v_accvgpr_read asm made the allocator spill in the steady k-steps: 1.57 -> 1.79 ms)
    if constexpr (C == 0) prev0[T] = acc0[T];
    else if constexpr (!ONE) st1[(T * 4 + C - 1) * 64] = make_float4(acc1[T][4 * (C - 1)], acc1[T][4 * (C - 1) + 1], acc1[T][4 * (C - 1) + 2], acc1[T][4 * (C - 1) + 3]);
  }
  template <int C, int Q>
  __device__ __forceinline__ void conv() {
    if constexpr (ONE && Q >= 4) return;
    if constexpr (C == 0 && Q >= 4) { cv.v1[2 * (Q & 3)] = acc1[0][2 * (Q & 3)]; cv.v1[2 * (Q & 3) + 1] = acc1[0][2 * (Q & 3) + 1]; }
    cv.template chunk<C, Q>();
  }
  template <int C, int PI>
  __device__ __forceinline__ void chunk() {
    if constexpr (PI >= 1) {
      move<C, PI - 1>();
      conv<C, PI - 1>();
      // pair 7 after pair 6 (PrevConv keeps ONE pair in flight: x0 / x1)
      if constexpr (PI == 7 && C == 4) { conv<0, 7>(); conv<1, 7>(); conv<2, 7>(); conv<3, 7>(); conv<4, 7>(); }
    }
  }
  __device__ __forceinline__ void finish() {
    move<0, 7>(); move<1, 7>(); move<2, 7>(); move<3, 7>(); move<4, 7>();
  }
};


// one n-tile of one k-step: 6 (X3) or 2 MFMAs with the conversion chunks of pair PI in their shadow
// PASSES (X3 modes): 3 = hi*hi + hi*lo + lo*hi (fp32-grade), 2 = drop the lo(weight) term, 1 = hi*hi only
template <int PREC, bool FIRST, int PI, typename W, int PASSES = Prec<PREC>::PASSES, typename BOPS = KOps>
__device__ __forceinline__ void tile_mfma(f32x16& a0, f32x16& a1, const uint4 ah, const uint4 al, const BOPS& b, W& work) {
  using PP = Prec<PREC>;
  constexpr bool TWO = !BOPS::ONE;      // m-tile 1 exists
  const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  a0 = mfma16<PP::F16>(ah, b.h0, FIRST ? zero : a0);
  work.template chunk<0, PI>();
  RNERF_PIN();
  if constexpr (TWO) a1 = mfma16<PP::F16>(ah, b.h1, FIRST ? zero : a1);
  work.template chunk<1, PI>();
  RNERF_PIN();
  if constexpr (PP::NP == 2 && PASSES == 3) {
    a0 = mfma16<PP::F16>(ah, b.l0, a0);
    work.template chunk<2, PI>();
    RNERF_PIN();
    if constexpr (TWO) a1 = mfma16<PP::F16>(ah, b.l1, a1);
    work.template chunk<3, PI>();
    RNERF_PIN();
    a0 = mfma16<PP::F16>(al, b.h0, a0);
    work.template chunk<4, PI>();
    RNERF_PIN();
    if constexpr (TWO) a1 = mfma16<PP::F16>(al, b.h1, a1);
  } else if constexpr (PP::NP == 2 && PASSES == 38) {      // f16 main term + the two cross terms on the fp8 MFMA
    a0 = mfma_f8(al.x, al.y, b.l0.x, b.l0.y, a0);            // fp8(W_lo) * fp8(x)
    work.template chunk<2, PI>();
    RNERF_PIN();
    if constexpr (TWO) a1 = mfma_f8(al.x, al.y, b.l1.x, b.l1.y, a1);
    work.template chunk<3, PI>();
    RNERF_PIN();
    a0 = mfma_f8(al.z, al.w, b.l0.z, b.l0.w, a0);            // fp8(W 2^-10) * fp8(x_lo 2^10)
    work.template chunk<4, PI>();
    RNERF_PIN();
    if constexpr (TWO) a1 = mfma_f8(al.z, al.w, b.l1.z, b.l1.w, a1);
  } else if constexpr (PP::NP == 2 && PASSES == 2) {
    a0 = mfma16<PP::F16>(ah, b.l0, a0);
    work.template chunk<2, PI>();
    work.template chunk<3, PI>();
    RNERF_PIN();
    if constexpr (TWO) a1 = mfma16<PP::F16>(ah, b.l1, a1);
    work.template chunk<4, PI>();
  } else if constexpr (PP::NP == 2 && PASSES == 22) {      // (W_hi + W_lo) * x_hi: the operand is a single 16-bit part
    a0 = mfma16<PP::F16>(al, b.h0, a0);
    work.template chunk<2, PI>();
    work.template chunk<3, PI>();
    RNERF_PIN();
    if constexpr (TWO) a1 = mfma16<PP::F16>(al, b.h1, a1);
    work.template chunk<4, PI>();
  } else {
    work.template chunk<2, PI>();
    work.template chunk<3, PI>();
    work.template chunk<4, PI>();
  }
  RNERF_PIN();
}

// one k-step (block KOFF of the slab) of MFMAs for NT n-tiles x 2 m-tiles; FIRST: accumulators start from 0.
// The A fragments of tile t+1 are read from LDS before the MFMAs of tile t are issued.
struct NoDma { __device__ __forceinline__ void operator()() const {} };
// The training kernels' four operand / gradient stores of a k-step stay at its head, in front of the first MFMA.  Spread behind tiles
// 2..5 instead (in the MFMAs' shadow, like the conversion chunks) they measured no faster in the training forward and slower in the dgrad
// (1.771 / 1.783 -> 1.838 / 1.842 ms, its spills grow from 259 to 301 registers; DESIGN.md section 3.3, profiles/r06/README.md).

// `dma` is invoked after tile 1: the weight DMA of the next slab is issued while MFMAs are already in the matrix pipe and
// the A fragments of tiles 0..3 are already on their way (an LDS-DMA instruction costs ~100 issue cycles).
// A fragments are read FRAG_DEPTH tiles ahead of their MFMAs: with one wave per SIMD the LDS read rate is set by the
// number of reads in flight (latency x concurrency), not by the 256 B/clk peak.
constexpr int FRAG_DEPTH = 4;

template <int PREC, int NT, int KOFF, bool FIRST, typename W, typename D = NoDma, int PASSES = Prec<PREC>::PASSES, typename BOPS = KOps>
__device__ __forceinline__ void kstep_mfma(f32x16 (&acc0)[8], f32x16 (&acc1)[8], const BOPS& b, const char* slab, int lane, W& work, D dma = D()) {
  using PP = Prec<PREC>;
  const uint4* a = (const uint4*)slab + lane + (size_t)KOFF * NT * PP::NP * 64;
  uint4 fh[FRAG_DEPTH], fl[FRAG_DEPTH];
  // second block of a tile: 16 bytes per lane; f16f8: two 8-byte planes [fp8(W_lo): 64 lanes][fp8(W 2^-10): 64 lanes], read as two
  // conflict-free 8-byte loads (read as one 16-byte value whose halves are used at different times, hipcc re-reads the first half later
  // with a second, narrower load right in front of its MFMA)
  auto load_lo = [&](int tile) -> uint4 {
    if constexpr (PP::F8X) {
      const uint2* a2 = (const uint2*)((const uint4*)slab + ((size_t)KOFF * NT + tile) * PP::NP * 64 + 64) + lane;
      const uint2 u = a2[0], v = a2[64];
      return make_uint4(u.x, u.y, v.x, v.y);
    } else return a[(tile * PP::NP + PP::NP - 1) * 64];
  };
#pragma unroll
  for (int t = 0; t < FRAG_DEPTH; ++t) {
    const int tt = t < NT ? t : NT - 1;
    fh[t] = a[(tt * PP::NP) * 64];
    fl[t] = load_lo(tt);
  }
#define RNERF_TILE(T)                                                                                     \
  if constexpr (T < NT) {                                                                                 \
    const uint4 ah = fh[T % FRAG_DEPTH], al = fl[T % FRAG_DEPTH];                                         \
    tile_mfma<PREC, FIRST, (T & 7), W, PASSES, BOPS>(acc0[T], acc1[T], ah, al, b, work);                  \
    if constexpr (T + FRAG_DEPTH < NT) {                                                                  \
      fh[T % FRAG_DEPTH] = a[((T + FRAG_DEPTH) * PP::NP) * 64];                                           \
      fl[T % FRAG_DEPTH] = load_lo(T + FRAG_DEPTH);                                                       \
    }                                                                                                     \
  }
  RNERF_TILE(0) RNERF_TILE(1)
  dma();
  RNERF_TILE(2)
  if constexpr (NT == 8) RNERF_PIN();      // scheduling boundaries behind tiles 2..5: the measured schedules of the 8-tile k-steps depend on them
  RNERF_TILE(3)
  if constexpr (NT == 8) RNERF_PIN();
  RNERF_TILE(4)
  if constexpr (NT == 8) RNERF_PIN();
  RNERF_TILE(5)
  if constexpr (NT == 8) RNERF_PIN();
  RNERF_TILE(6) RNERF_TILE(7)
#undef RNERF_TILE
}

// Workgroup = 4 waves = 256 consecutive sample rows; wave w owns rows [64w, 64w+64) as two 32-row m-tiles.
//   registers : acc0/acc1 (fp32 accumulators of both m-tiles, 2 x 128), prev0 (fp32 outputs of the previous layer, m-tile 0)
//   LDS       : 2 x SLAB weight ring (shared by the 4 waves) + 32 KiB per wave holding the previous layer's fp32 outputs
//               of m-tile 1 ([n-tile][4-register group][lane] float4) = 160 KiB for the X3 modes.
// The previous layer's outputs become this layer's B operands JUST IN TIME, one k-step ahead of use: bias + ReLU +
// hi/lo split of 8 values per lane per m-tile, issued in the shadow of the 48 MFMAs of the current k-step.
// Saved-activation layout of the training forward (consumed by the dgrad / wgrad kernels): slot-major uint4[SAVE_SLOTS][R][2]
// (R = rows padded to the 256-row tile), one uint4 = the 8 hi-part operand values lane (row, half h) fed to one k-step, i.e.
// exactly the B operands of the forward MFMAs.  slot 0..3: position encoding; 4 + 16*(l-1) + s: input k-step s of MFMA layer
// l = 1..9; 148..149: view encoding; 150..157: ReLU'd output of the view layer (= rgb head input).
// slots 158..166: ReLU bit masks for the dgrad chain, one uint4 per (row, half) per mask set (set l-1 = the input of MFMA layer
// l = 1..8, set 8 = the rgb-head input), stored word-major uint32[9][4][R][2]: word w holds k-steps 4w..4w+3 (written as soon as
// they are converted: no register lives across the layer), byte s&3, bit (j>>1) + 4*(j&1) <=> element j of k-step s is non-zero.
constexpr int SAVE_PE = 0, SAVE_L1 = 4, SAVE_VIEW = 148, SAVE_RGBIN = 150, SAVE_SLOTS = 158, SAVE_MASK = 158, SAVE_TOTAL = 167;
// Memory layout of the saved operands (and of the dY planes below): TILE-major — [32-row tile][slot][row in tile][half] uint4, so that
// the slots a wave touches for its 32 rows are consecutive 1 KiB blocks: the training forward / the dgrad write, and the wgrad reads,
// 16-32 KiB contiguous per (wave, chunk) instead of 1 KiB pieces 16 MB apart (one DRAM page activation per KiB).  The save buffer is
// [hi plane: SAVE_SLOTS slots][ReLU masks: 36 dword-slots = 576 uint4 per tile][lo plane: SAVE_SLOTS slots (hi + lo mode only)].
__host__ __device__ constexpr size_t sv_mask0(long long R) { return (size_t)(R / 32) * SAVE_SLOTS * 64; }                  // uint4 units
__host__ __device__ constexpr size_t sv_lo0(long long R) { return sv_mask0(R) + (size_t)(R / 32) * 576; }
__host__ __device__ constexpr size_t sv_addr(int q, long long t32, int m, int h) { return (((size_t)t32 * SAVE_SLOTS + q) * 32 + m) * 2 + h; }
__host__ __device__ constexpr size_t sv_mask_addr(int sw, long long t32, int m, int h) { return (((size_t)t32 * 36 + sw) * 32 + m) * 2 + h; }   // dword units

// non-zero flags of the 8 post-ReLU (non-negative) 16-bit values of one operand: bits 0..3 = even elements, 16..19 = odd elements
__device__ __forceinline__ uint32_t nz_nibbles(const uint4& o) {
  return pk_min1(o.x) | (pk_min1(o.y) << 1) | (pk_min1(o.z) << 2) | (pk_min1(o.w) << 3);
}
__device__ __forceinline__ uint32_t nz_byte(uint32_t nib) { return (nib & 0xFu) | (nib >> 12); }   // even flags | odd flags << 4

// TRAIN: 0 = evaluation, 1 = training forward keeping the hi 16-bit operand parts, 2 = hi and lo parts (fp32-grade backward),
// 3 = hi parts + the lo parts as e4m3 bytes (RNERF_BWD_F16X3_LO8: lo8 plane = uint2[...] at the lo plane's place, same (tile, slot, row, half) order)
template <int PREC, int MODE, int TRAIN, bool ONE = false>
__global__ void __launch_bounds__(256, 1)
nerfmlp_fwd_kernel(const char* __restrict__ packed, const float4* __restrict__ rows_pd, const float4* __restrict__ rows_dr,
                   const int* __restrict__ node_of_sample, int B, long long total_rows, int n_tiles, float4* __restrict__ out_raw,
                   uint4* __restrict__ save, long long save_rows, int* __restrict__ tileq, const float* __restrict__ gate, int gate_skip_if) {
  // gate (nullable): a range flag raised by a pack kernel.  The launch does nothing when (flag set) == gate_skip_if: the f16f8 forward steps
  // aside when one of ITS weights left the range of its 2^14-scaled stream, and the f16x3 launch queued right behind it (same outputs,
  // gate_skip_if = 0) does the work instead — a per-launch fallback decided on the device, no host round trip (rnerf_nerfmlp_forward).
  if (gate != nullptr && ((gate[0] != 0.f) == (gate_skip_if != 0))) return;
  // tileq != nullptr (training forward on a capped grid): tiles beyond the first round are handed out by an atomic counter (tileq[0],
  // zeroed by the launcher; tileq[1 + workgroup] passes the draw from thread 0 to the other waves) — with fewer workgroups than CUs the
  // static stride would leave most of the chip idle in a last partial round (2048 tiles over 248 workgroups: 9 rounds instead of 8.26).
  // ONE: 128-row tiles — every wave runs ONE 32-row m-tile (rows 128 tile + 32 wave + m): half the serial work per tile, for launches whose
  // 256-row tiles would leave more than half of the CUs idle.  n_tiles then counts 128-row tiles; the save layout (32-row tiles) is the same.
  using PP = Prec<PREC>;
  using KOps = KOpsT<ONE>;
  constexpr int SLAB = PP::SLAB;
  constexpr int WROWS = ONE ? 32 : 64, TROWS = 4 * WROWS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr bool OVFL_MODE = PP::F8X || TRAIN == 3;      // fp8 conversions clamp; f16 overflow clamps to 65504 too (see `watch`)
  if constexpr (OVFL_MODE) f8x_mode();
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 31, h = lane >> 5;
  const float* __restrict__ aux = (const float*)(packed + PP::STREAM_BYTES);
  float4* __restrict__ st1 = (float4*)(smem + 2 * SLAB + wave * 32768) + lane;   // + (t*4 + rq)*64
  constexpr float INV_SCALE = 1.0f / PP::WSCALE;
  int buf = 0;
  size_t off = 0;   // stream offset of the next slab to prefetch
  // One shader-clock read, result unused: every measured build of this kernel has it here, so it stays until a timing A/B retires it.
  (void)__builtin_amdgcn_s_memtime();

  // MODE 512 — REDO, the range-safe second pass (rnerf_nerfmlp_forward queues it behind every f16-based evaluation launch, in bf16x3: fp32's
  // exponent range): it walks the same tiles but works only on those that hold a row the first pass returned as NaN (an activation above
  // f16's 65504 or a weight >= 256, see `watch` / AUX_FLAG below) and rewrites only those rows.  The flags ARE the first pass's outputs: no
  // scratch, nothing to clear, and a launch without such a row costs one read of out_raw (8 tiles' rows in flight per barrier).
  // (MODE is a template parameter, not a bool, because it is part of the kernels' names.)
  constexpr bool REDO = (MODE & 512) != 0;
  // bit k of `todo`: this workgroup's k-th tile (blockIdx.x + k gridDim.x) holds a NaN row.  Found in the prologue, while the LDS is still
  // free (four 8-byte words for the cross-wave OR; the kernel owns all 160 KiB later).  A workgroup with more than 64 tiles works on every
  // tile beyond the 64th (correct — only NaN rows are rewritten — just not skipped: > 4 M rows per launch on this chip).
  unsigned long long todo = ~0ull;
  if constexpr (REDO) {
    unsigned long long mine = 0;
#pragma unroll 8
    for (int k = 0; k < 64; ++k) {
      const long long tk = (long long)blockIdx.x + (long long)k * gridDim.x;
      const long long r = tk * TROWS + tid;
      const bool bad = tk < n_tiles && r < total_rows && __builtin_isnan(out_raw[r].x);
      if (__ballot(bad) != 0ull) mine |= 1ull << k;
    }
    unsigned long long* red = (unsigned long long*)smem;
    if (lane == 0) red[wave] = mine;
    __syncthreads();
    todo = red[0] | red[1] | red[2] | red[3];
    __syncthreads();
  }
  auto find_next = [&](int t) -> int {      // first tile >= t of this workgroup's sequence that is to be worked on; n_tiles if none
    if constexpr (REDO) {
      while (t < n_tiles) {
        const int k = (t - (int)blockIdx.x) / (int)gridDim.x;
        if (k >= 64 || ((todo >> k) & 1ull)) return t;
        t += (int)gridDim.x;
      }
      return n_tiles;
    } else {
      return t;
    }
  };
  const int first_tile = find_next((int)blockIdx.x);
  if (first_tile < n_tiles) { issue_slab<SLAB>(packed, 0u, wave, lane); off = SLAB; }
  slab_wait_dma();
  __syncthreads();

  for (int tile = first_tile; tile < n_tiles;) {
    if (tileq != nullptr && tid == 0)      // read back by every wave at the end of the tile, ~145 barriers later
      __hip_atomic_store(tileq + 1 + blockIdx.x, (int)gridDim.x + atomicAdd(tileq, 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // The aux vectors (biases, head weights) are read at lane-dependent but tile-invariant addresses.  Left alone, hipcc hoists the ~100
    // 64-bit per-lane addresses out of the tile loop, spills them, and in the heads / the view layer reloads each one from scratch right
    // before its load, one after the other (measured: 52 k clocks for the rgb head, 5.4 k per view-layer slab).  An opaque per-tile copy
    // of the base keeps the address arithmetic next to the loads (scalar base + lane offset + immediate).
    const float* __restrict__ auxt = aux;
    asm volatile("" : "+s"(auxt));
    int next_tile = n_tiles;
    long long row[2]; bool row_ok[2];
    float4 pd[2], dr[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      if (ONE && mt == 1) { row[1] = row[0]; row_ok[1] = false; pd[1] = pd[0]; dr[1] = dr[0]; continue; }
      row[mt] = (long long)tile * TROWS + wave * WROWS + mt * 32 + m;
      row_ok[mt] = row[mt] < total_rows;
      if (!row_ok[mt]) row[mt] = total_rows - 1;
      size_t rec = (size_t)row[mt];
      if (node_of_sample) { const long long sidx = row[mt] / B; rec = (size_t)node_of_sample[sidx] * B + (size_t)(row[mt] - sidx * B); }
      pd[mt] = rows_pd[rec];
      dr[mt] = rows_dr[rec];
    }

    f32x16 acc0[8], acc1[8], prev0[8];

    // training forward: keep the hi parts of the operands of slot q (see SAVE_* above); padded rows are written too
    const long long t32_0 = (long long)tile * (TROWS / 32) + wave * (WROWS / 32);      // 32-row tile of m-tile 0 (m-tile 1: + 1)
    auto save_ops = [&](int q, const KOps& o) {
      if constexpr (TRAIN != 0) {
        uint4* dst = save + sv_addr(q, t32_0, m, h);
        stream_store(dst, o.h0);
        if constexpr (!ONE) stream_store(dst + (size_t)SAVE_SLOTS * 64, o.h1);          // m-tile 1 = the next 32-row tile
        if constexpr (TRAIN == 2) {            // lo plane
          uint4* dl = dst + sv_lo0(save_rows);
          stream_store(dl, o.l0);
          if constexpr (!ONE) stream_store(dl + (size_t)SAVE_SLOTS * 64, o.l1);
        }
        if constexpr (TRAIN == 3) {            // lo plane as e4m3 bytes: 8 B per (row, half)
          uint2* dl = (uint2*)(save + sv_lo0(save_rows)) + sv_addr(q, t32_0, m, h);
          stream_store8(dl, lo8_pack<false>(o.l0, LO8_SCALE_X));
          if constexpr (!ONE) stream_store8(dl + (size_t)SAVE_SLOTS * 64, lo8_pack<false>(o.l1, LO8_SCALE_X));
        }
      }
    };

    // Range watch of the f16 operand parts.  A hidden activation above f16's 65504 becomes hi = inf; the next
    // layer's sums are inf - inf = NaN (sign bit set on this hardware), which the ReLU turns into 0 — every unit of that layer would read 0
    // and the outputs would be finite, plausible and wrong (found in round 4; DESIGN.md section 3.2, "Range").  So the largest |hi| bit pattern per lane
    // is kept (one v_pk_max_u16 per operand dword: positive f16 order like their bits, inf = 0x7C00) and a row that met inf / NaN returns NaN.
    uint32_t ovf0 = 0, ovf1 = 0;
    auto watch = [&](const KOps& o, bool is_signed) {      // (bf16 modes too — round 5: a non-finite position used to come out FINITE there)
      const uint32_t am = is_signed ? 0x7FFF7FFFu : 0xFFFFFFFFu;      // the bottleneck has no ReLU: drop the sign bits
      ovf0 = pk_maxu(pk_maxu(ovf0, o.h0.x & am), pk_maxu(pk_maxu(o.h0.y & am, o.h0.z & am), o.h0.w & am));
      if constexpr (!ONE) ovf1 = pk_maxu(pk_maxu(ovf1, o.h1.x & am), pk_maxu(pk_maxu(o.h1.y & am, o.h1.z & am), o.h1.w & am));
    };

    uint32_t mw0 = 0, mw1 = 0;                                                // mask bytes of up to 4 k-steps, then one dword store
    auto save_mask = [&](int set, int s, uint32_t nib0, uint32_t nib1) {      // nib: nz_nibbles() of the hi operands of k-step s
      if constexpr (TRAIN != 0) {
        if ((s & 3) == 0) { mw0 = nz_byte(nib0); mw1 = nz_byte(nib1); }
        else { mw0 |= nz_byte(nib0) << (8 * (s & 3)); mw1 |= nz_byte(nib1) << (8 * (s & 3)); }
        if ((s & 3) == 3) {      // word-major: a wave's 64 dwords are contiguous (full-line writes)
          uint32_t* dst = (uint32_t*)(save + sv_mask0(save_rows)) + sv_mask_addr(set * 4 + (s >> 2), t32_0, m, h);
          __builtin_nontemporal_store(mw0, dst);
          if constexpr (!ONE) __builtin_nontemporal_store(mw1, dst + 36 * 64);
        }
      }
    };

    // positional-encoding operands of k-step s (slot maps pe_feature / view_feature), for both m-tiles
    auto enc_ops = [&](const float4 (&v)[2], int s, int nsin) -> KOps {
      const float phase = h ? 1.5707963705062866f : 0.0f;   // f32(0.5*pi) (rnerf/model_utils.py:213)
      float f[2][8];
#pragma unroll
      for (int mt = 0; mt < (ONE ? 1 : 2); ++mt)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int q = 8 * s + j;
          if (q < nsin) {
            const int d = q / 3, c = q % 3;
            const float x = c == 0 ? v[mt].x : (c == 1 ? v[mt].y : v[mt].z);
            f[mt][j] = pe_sin(fadd(fmul(x, (float)(1 << d)), phase));
          } else if (q == nsin) f[mt][j] = h ? v[mt].z : v[mt].x;
          else if (q == nsin + 1) f[mt][j] = h ? 0.f : v[mt].y;
          else f[mt][j] = 0.f;
        }
      KOps o;
      split8<PREC>(f[0], o.h0, o.l0);
      if constexpr (ONE) { o.h1 = o.h0; o.l1 = o.l0; } else split8<PREC>(f[1], o.h1, o.l1);
      return o;
    };

    // operands of k-step s from the previous layer's outputs: x = max(acc * inv_scale + bias, floor), hi/lo split.
    auto prev_ops = [&](int s, const float* __restrict__ bias, int floor_v) -> KOps {
      const float4 b0 = *(const float4*)(bias + 16 * s + 4 * h), b1 = *(const float4*)(bias + 16 * s + 8 + 4 * h);
      const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
      float r1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if constexpr (!ONE) {
        const float4 u0 = st1[((s >> 1) * 4 + 2 * (s & 1)) * 64], u1 = st1[((s >> 1) * 4 + 2 * (s & 1) + 1) * 64];
        r1[0] = u0.x; r1[1] = u0.y; r1[2] = u0.z; r1[3] = u0.w; r1[4] = u1.x; r1[5] = u1.y; r1[6] = u1.z; r1[7] = u1.w;
      }
      float x0[8], x1[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        x0[j] = relu_keep(fmaf(prev0[s >> 1][8 * (s & 1) + j], INV_SCALE, bb[j]), floor_v);
        x1[j] = relu_keep(fmaf(r1[j], INV_SCALE, bb[j]), floor_v);
      }
      KOps o;
      split8<PREC>(x0, o.h0, o.l0);
      if constexpr (ONE) { o.h1 = o.h0; o.l1 = o.l0; } else split8<PREC>(x1, o.h1, o.l1);
      return o;
    };

    // bias of the 8 features of k-step s (global, L2/L1 resident).  Loaded one slab EARLIER than it is consumed: the
    // vmcnt(0) of the barrier that ends the slab (needed for the weight DMA anyway) then also covers this load.
    auto load_bias8 = [&](int s, const float* __restrict__ bias, float (&b)[8]) {
      const float4 b0 = *(const float4*)(bias + 16 * s + 4 * h), b1 = *(const float4*)(bias + 16 * s + 8 + 4 * h);
      b[0] = b0.x; b[1] = b0.y; b[2] = b0.z; b[3] = b0.w; b[4] = b1.x; b[5] = b1.y; b[6] = b1.z; b[7] = b1.w;
    };
    // raw accumulators of m-tile 1 for k-step s (this wave's LDS region)
    auto load_state8 = [&](int s, float (&v)[8]) {
      if constexpr (ONE) return;
      const float4 u0 = st1[((s >> 1) * 4 + 2 * (s & 1)) * 64], u1 = st1[((s >> 1) * 4 + 2 * (s & 1) + 1) * 64];
      v[0] = u0.x; v[1] = u0.y; v[2] = u0.z; v[3] = u0.w; v[4] = u1.x; v[5] = u1.y; v[6] = u1.z; v[7] = u1.w;
    };
    NoWork nowork;

#define SLAB_PREFETCH(DO_NEXT)                                                                                       \
  do { if (DO_NEXT) { issue_slab<SLAB>(packed + off, (unsigned)((buf ^ 1) * SLAB), wave, lane); off += SLAB; } } while (0)
#define SLAB_DONE() do { slab_wait_dma(); __syncthreads(); buf ^= 1; } while (0)

    float sig0 = 0.f, sig1 = 0.f;

    // ---- layer 0: pos_enc(pos, 0, 10) (63) -> 256 (Dense_0)  (rnerf/models.py:257)
    KOps cur;                                   // operands of the next k-step; across a layer seam: k-step 0 of the next layer (SeamWork)
    {
      cur = enc_ops(pd, 0, 30);
      SeamWork<PREC, TRAIN != 0, ONE> seam(acc0, acc1, prev0, st1);
      seam.cv.floor_v = RELU_FLOOR;
      load_bias8(0, auxt + AUX_BIAS, seam.cv.b);
      load_bias8(0, auxt + AUX_ZERO, seam.cv.ws);
      // k-steps 0..2 convert the position-encoding operands of the next k-step in their own MFMA shadows (EncWork), k-step 3 carries the seam
#define RNERF_PE_KSTEP(S, FIRST_, SAVE_)                                                                             \
      {                                                                                                              \
        if (SAVE_) save_ops(SAVE_PE + S, cur);                                                                       \
        watch(cur, true);      /* a non-finite position (a caller's NaN) must not come out as a colour either */    \
        SLAB_PREFETCH(true);   /* glds first: it is a scheduling boundary, conversion + MFMAs must share the region after it */ \
        if constexpr (S < 3) {                                                                                       \
          EncWork<PREC, S + 1, 30, ONE> ew(pd, h);                                                                        \
          kstep_mfma<PREC, 8, 0, FIRST_>(acc0, acc1, cur, smem + buf * SLAB, lane, ew);                              \
          cur = ew.result();                                                                                         \
        } else {                                                                                                     \
          kstep_mfma<PREC, 8, 0, false>(acc0, acc1, cur, smem + buf * SLAB, lane, seam);                             \
        }                                                                                                            \
        SLAB_DONE();                                                                                                 \
      }
      RNERF_PE_KSTEP(0, true, true) RNERF_PE_KSTEP(1, false, true) RNERF_PE_KSTEP(2, false, true) RNERF_PE_KSTEP(3, false, true)
      seam.finish();
      cur = seam.cv.result();
    }

    // bias / sigma weights of the conversion that runs in the shadow of the next hidden k-step (fetched one slab ahead, across layers too)
    float bnext[8], wnext[8];
    load_bias8(1, auxt + AUX_BIAS, bnext);
    load_bias8(1, auxt + AUX_ZERO, wnext);

    // ---- layers 1..8: Dense_1..Dense_7 (inputs ReLU'd; Dense_5 also takes the skip concat), Dense_9 = bottleneck
#pragma unroll 1
    for (int l = 1; l <= 8; ++l) {
      const float* __restrict__ bias = auxt + AUX_BIAS + 256 * (l - 1);
      // the seam of this layer: hand-over of the outputs + conversion of the next layer's k-step 0 (bias of THIS layer; the bottleneck
      // Dense_9 = layer 8 has no activation), run by the layer's last k-step
      SeamWork<PREC, TRAIN != 0, ONE> seam(acc0, acc1, prev0, st1);
      seam.cv.floor_v = l == 8 ? NO_FLOOR : RELU_FLOOR;
      // sigma head (Dense_8, rnerf/model_utils.py:70) = sum over the trunk output x7 = the inputs of layer 8: k-step 0 in layer 7's seam,
      // k-steps 1..15 in layer 8's conversions.  (The seam's bias / sigma weights are fetched at k-step 13: 16 registers less in the steady state.)
      const float* __restrict__ wseam = auxt + (l == 7 ? AUX_WSIG : AUX_ZERO);
      const float* __restrict__ wsel = auxt + (l == 8 ? AUX_WSIG : AUX_ZERO);
#define RNERF_KSTEP(S)                                                                                              \
      {                                                                                                              \
        save_ops(SAVE_L1 + 16 * (l - 1) + S, cur);                                                                   \
        watch(cur, false);                                                                                           \
        if constexpr (TRAIN != 0 && S == 0) save_mask(l - 1, 0, nz_nibbles(cur.h0), nz_nibbles(cur.h1));                  \
        if constexpr (S == 13) { load_bias8(0, bias + 256, seam.cv.b); load_bias8(0, wseam, seam.cv.ws); }           \
        float bnn[8], wnn[8];                                                                                        \
        if constexpr (S + 2 < 16) { load_bias8(S + 2, bias, bnn); load_bias8(S + 2, wsel, wnn); }   /* consumed in the NEXT slab */ \
        else if constexpr (S == 14) { load_bias8(1, bias + 256, bnn); load_bias8(1, wseam, wnn); }   /* k-step 1 of the NEXT layer */ \
        auto dma = [&]() { SLAB_PREFETCH(true); };                                                                   \
        if constexpr (S + 1 < 16) {                                                                                  \
          PrevConv<PREC, S + 1, TRAIN != 0, true, ONE> cv(prev0[(S + 1) >> 1]);                                           \
          cv.floor_v = RELU_FLOOR;                                                                                        \
          _Pragma("unroll") for (int j = 0; j < 8; ++j) { cv.b[j] = bnext[j]; cv.ws[j] = wnext[j]; }                 \
          load_state8(S + 1, cv.v1);                                                                                 \
          kstep_mfma<PREC, 8, 0, S == 0, PrevConv<PREC, S + 1, TRAIN != 0, true, ONE>, decltype(dma)>(acc0, acc1, cur, smem + buf * SLAB, lane, cv, dma); \
          cur = cv.result();                                                                                         \
          sig0 += cv.sg0; sig1 += cv.sg1;                                                                            \
          save_mask(l - 1, S + 1, cv.nz[0], cv.nz[1]);                                                               \
        } else {                                                                                                     \
          /* also for l == 5, whose last k-step is the 4th skip slab: that one runs the seam again on the final sums (no branch here: */ \
          /* a run-time choice of the work functor splits the accumulators' live ranges and hipcc spills them around it) */ \
          kstep_mfma<PREC, 8, 0, false, SeamWork<PREC, TRAIN != 0, ONE>, decltype(dma)>(acc0, acc1, cur, smem + buf * SLAB, lane, seam, dma); \
        }                                                                                                            \
        if constexpr (S + 2 <= 16) { _Pragma("unroll") for (int j = 0; j < 8; ++j) { bnext[j] = bnn[j]; wnext[j] = wnn[j]; } } \
        SLAB_DONE();                                                                                                 \
      }
      RNERF_KSTEP(0) RNERF_KSTEP(1) RNERF_KSTEP(2) RNERF_KSTEP(3) RNERF_KSTEP(4) RNERF_KSTEP(5) RNERF_KSTEP(6) RNERF_KSTEP(7)
      RNERF_KSTEP(8) RNERF_KSTEP(9) RNERF_KSTEP(10) RNERF_KSTEP(11) RNERF_KSTEP(12) RNERF_KSTEP(13) RNERF_KSTEP(14) RNERF_KSTEP(15)
#undef RNERF_KSTEP
      if (l == 5) {   // skip concat: [x, inputs] (rnerf/model_utils.py:68-69)
        // the encoding is recomputed here on purpose (in the MFMA shadow); with the position opaque the compiler cannot keep layer 0's
        // encoded values alive across five layers instead (f16f8: it kept all 64, through scratch — 8 k clocks per skip slab instead of 4)
        asm volatile("" : "+v"(pd[0].x), "+v"(pd[0].y), "+v"(pd[0].z), "+v"(pd[1].x), "+v"(pd[1].y), "+v"(pd[1].z));
        cur = enc_ops(pd, 0, 30);
        RNERF_PE_KSTEP(0, false, false) RNERF_PE_KSTEP(1, false, false) RNERF_PE_KSTEP(2, false, false) RNERF_PE_KSTEP(3, false, false)
      }
      seam.finish();
      cur = seam.cv.result();
      sig0 += seam.cv.sg0; sig1 += seam.cv.sg1;
    }

    // ---- view layer: [bottleneck(256) (no activation), pos_enc(dir, 0, 4) (27)] -> 128 (Dense_10)  (rnerf/models.py:289-294)
    {
      const float* __restrict__ bias = auxt + AUX_BIAS + 256 * 8;
      KOps c0 = cur;                             // converted by layer 8's seam
      KOps c1 = prev_ops(1, bias, NO_FLOOR);
      float bA[8], bB[8];                        // biases of the two k-steps converted in the shadow of the current slab
      load_bias8(2, bias, bA);
      load_bias8(3, bias, bB);
#define RNERF_VSLAB(SL)                                                                                              \
      {                                                                                                              \
        save_ops(SAVE_L1 + 16 * 8 + 2 * SL, c0);                                                                     \
        save_ops(SAVE_L1 + 16 * 8 + 2 * SL + 1, c1);                                                                 \
        watch(c0, true); watch(c1, true);                                                                            \
        SLAB_PREFETCH(true);                                                                                         \
        if constexpr (SL + 1 < 8) {                                                                                  \
          float bA2[8], bB2[8];                                                                                      \
          if constexpr (SL + 2 < 8) { load_bias8(2 * SL + 4, bias, bA2); load_bias8(2 * SL + 5, bias, bB2); }        \
          PrevConv<PREC, 2 * SL + 2, false, false, ONE> cvA(prev0[SL + 1]);                                                      \
          PrevConv<PREC, 2 * SL + 3, false, false, ONE> cvB(prev0[SL + 1]);                                                      \
          cvA.floor_v = NO_FLOOR; cvB.floor_v = NO_FLOOR;                                                                \
          _Pragma("unroll") for (int j = 0; j < 8; ++j) { cvA.b[j] = bA[j]; cvB.b[j] = bB[j]; }                      \
          load_state8(2 * SL + 2, cvA.v1);                                                                           \
          load_state8(2 * SL + 3, cvB.v1);                                                                           \
          PairOfPairs<decltype(cvA)> wA(cvA);                                                                        \
          PairOfPairs<decltype(cvB)> wB(cvB);                                                                        \
          kstep_mfma<PREC, 4, 0, SL == 0>(acc0, acc1, c0, smem + buf * SLAB, lane, wA);                              \
          kstep_mfma<PREC, 4, 1, false>(acc0, acc1, c1, smem + buf * SLAB, lane, wB);                                \
          c0 = cvA.result(); c1 = cvB.result();                                                                      \
          if constexpr (SL + 2 < 8) { _Pragma("unroll") for (int j = 0; j < 8; ++j) { bA[j] = bA2[j]; bB[j] = bB2[j]; } } \
        } else {                                                                                                     \
          const KOps n0 = enc_ops(dr, 0, 12), n1 = enc_ops(dr, 1, 12);                                               \
          kstep_mfma<PREC, 4, 0, false>(acc0, acc1, c0, smem + buf * SLAB, lane, nowork);                            \
          kstep_mfma<PREC, 4, 1, false>(acc0, acc1, c1, smem + buf * SLAB, lane, nowork);                            \
          c0 = n0; c1 = n1;                                                                                          \
        }                                                                                                            \
        SLAB_DONE();                                                                                                 \
      }
      RNERF_VSLAB(0) RNERF_VSLAB(1) RNERF_VSLAB(2) RNERF_VSLAB(3) RNERF_VSLAB(4) RNERF_VSLAB(5) RNERF_VSLAB(6) RNERF_VSLAB(7)
#undef RNERF_VSLAB
      // last slab of the tile (the two view-encoding k-steps): prefetch the first slab of the next tile (stream restarts)
      save_ops(SAVE_VIEW, c0);
      save_ops(SAVE_VIEW + 1, c1);
      watch(c0, true); watch(c1, true);
      next_tile = tileq != nullptr ? __builtin_amdgcn_readfirstlane(__hip_atomic_load(tileq + 1 + blockIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                                   : find_next(tile + (int)gridDim.x);
      const bool has_next_tile = next_tile < n_tiles;
      if (has_next_tile) off = 0;
      SLAB_PREFETCH(has_next_tile);
      kstep_mfma<PREC, 4, 0, false>(acc0, acc1, c0, smem + buf * SLAB, lane, nowork);
      kstep_mfma<PREC, 4, 1, false>(acc0, acc1, c1, smem + buf * SLAB, lane, nowork);
      SLAB_DONE();
    }

    // ---- heads: sigma (Dense_8, accumulated above) and rgb (Dense_11) on the fp32 view-layer output
    {
      // the 16 weight / bias vectors of n-tile t + 1 are fetched while n-tile t is reduced (left to itself hipcc loads two vectors, waits,
      // uses them, loads the next two: 32 exposed round trips, 18 k clocks per tile)
      const float* __restrict__ hw = auxt + 4 * h;
      auto head_load = [&](int t, float4 (&W)[16]) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = 32 * t + 8 * g;
          W[4 * g] = gload4(hw + AUX_BIAS + 256 * 9 + n);
          W[4 * g + 1] = gload4(hw + AUX_WRGB + n); W[4 * g + 2] = gload4(hw + AUX_WRGB + 128 + n); W[4 * g + 3] = gload4(hw + AUX_WRGB + 256 + n);
        }
      };
      float p0[3] = {0.f, 0.f, 0.f}, p1[3] = {0.f, 0.f, 0.f};
      float4 Wc[16];
      head_load(0, Wc);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float4 Wn[16];
        if (t + 1 < 4) head_load(t + 1, Wn);
        RNERF_PIN();
        float rv0[16], rv1[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 bb = Wc[4 * g], wr = Wc[4 * g + 1], wg = Wc[4 * g + 2], wb = Wc[4 * g + 3];
          const float bv[4] = {bb.x, bb.y, bb.z, bb.w}, wrv[4] = {wr.x, wr.y, wr.z, wr.w}, wgv[4] = {wg.x, wg.y, wg.z, wg.w}, wbv[4] = {wb.x, wb.y, wb.z, wb.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float v0 = relu_keep(fmaf(acc0[t][4 * g + i], INV_SCALE, bv[i]), RELU_FLOOR);
            p0[0] = fmaf(v0, wrv[i], p0[0]); p0[1] = fmaf(v0, wgv[i], p0[1]); p0[2] = fmaf(v0, wbv[i], p0[2]);
            rv0[4 * g + i] = v0;
            if constexpr (!ONE) {
              const float v1 = relu_keep(fmaf(acc1[t][4 * g + i], INV_SCALE, bv[i]), RELU_FLOOR);
              p1[0] = fmaf(v1, wrv[i], p1[0]); p1[1] = fmaf(v1, wgv[i], p1[1]); p1[2] = fmaf(v1, wbv[i], p1[2]);
              rv1[4 * g + i] = v1;
            } else rv1[4 * g + i] = v0;
          }
        }
        if (t + 1 < 4) {
#pragma unroll
          for (int q = 0; q < 16; ++q) Wc[q] = Wn[q];
        }
        if constexpr (TRAIN != 0) {   // rgb-head input (ReLU'd view-layer output) in operand-slot order: k-step 2t + half, slot j = reg & 7
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            KOps o;
            float a0[8], a1[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { a0[j] = rv0[8 * half + j]; a1[j] = rv1[8 * half + j]; }
            if constexpr (TRAIN >= 2) { split8<PREC>(a0, o.h0, o.l0); split8<PREC>(a1, o.h1, o.l1); }
            else {
              o.h0 = make_uint4(pack2<PP::F16>(a0[0], a0[1]), pack2<PP::F16>(a0[2], a0[3]), pack2<PP::F16>(a0[4], a0[5]), pack2<PP::F16>(a0[6], a0[7]));
              o.h1 = make_uint4(pack2<PP::F16>(a1[0], a1[1]), pack2<PP::F16>(a1[2], a1[3]), pack2<PP::F16>(a1[4], a1[5]), pack2<PP::F16>(a1[6], a1[7]));
            }
            save_ops(SAVE_RGBIN + 2 * t + half, o);
            save_mask(8, 2 * t + half, nz_nibbles(o.h0), nz_nibbles(o.h1));
          }
        }
      }
      const float bsig = auxt[AUX_BSIG];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        p0[c] = p0[c] + __shfl_xor(p0[c], 32) + auxt[AUX_BRGB + c];
        p1[c] = p1[c] + __shfl_xor(p1[c], 32) + auxt[AUX_BRGB + c];
      }
      sig0 = sig0 + __shfl_xor(sig0, 32) + bsig;
      sig1 = sig1 + __shfl_xor(sig1, 32) + bsig;
      {      // an activation outside the operand type's range somewhere along this row's chain (either half of its features); bf16: inf / NaN only
        ovf0 = pk_maxu(ovf0, (uint32_t)__shfl_xor((int)ovf0, 32));
        ovf1 = pk_maxu(ovf1, (uint32_t)__shfl_xor((int)ovf1, 32));
        const float qn = __builtin_nanf("");
        // f16f8 runs with MODE.FP16_OVFL (f8x_mode: the fp8 conversions must clamp) — and that bit also makes every f16 conversion clamp an
        // overflow to 65504 (0x7BFF) instead of producing inf: the watch has to take the clamp value itself as "left the range" there (found
        // in round 5 by the second-pass test: hidden activations of 3e5 rendered finite, wrong colours in the default eval precision)
        // f16f8 also feeds fp8(x) into its W_lo cross term: an activation beyond e4m3's 448 is clamped there (a silent 2^-12 relative error per
        // product that compounds over the layers — measured 1e-2 RGB on hidden kernels x 4, round 6): the watch hands every row with an
        // operand >= 448 (0x5F00) to the range-safe second pass as well
        constexpr uint32_t OVF = PP::F8X ? 0x5F00u : (OVFL_MODE ? 0x7BFFu : (PP::F16 ? 0x7C00u : 0x7F80u));
        if ((ovf0 & 0xFFFFu) >= OVF || (ovf0 >> 16) >= OVF) { p0[0] = p0[1] = p0[2] = qn; sig0 = qn; }
        if ((ovf1 & 0xFFFFu) >= OVF || (ovf1 >> 16) >= OVF) { p1[0] = p1[1] = p1[2] = qn; sig1 = qn; }
      }
      if constexpr (PP::F16 && !PP::F8X) {      // a weight outside the range of this precision's operand stream (|W| >= 256): fail loudly, not plausibly
        if (auxt[AUX_FLAG] != 0.f) { const float qn = __builtin_nanf(""); p0[0] = p0[1] = p0[2] = qn; p1[0] = p1[1] = p1[2] = qn; sig0 = qn; sig1 = qn; }
      }
      if (h == 0) {
        if constexpr (REDO) {      // only the rows the first pass gave up on: every other row keeps the first pass's bits
          if (row_ok[0] && __builtin_isnan(out_raw[row[0]].x)) out_raw[row[0]] = make_float4(p0[0], p0[1], p0[2], sig0);
          if (row_ok[1] && __builtin_isnan(out_raw[row[1]].x)) out_raw[row[1]] = make_float4(p1[0], p1[1], p1[2], sig1);
        } else {
          if (row_ok[0]) out_raw[row[0]] = make_float4(p0[0], p0[1], p0[2], sig0);
          if (row_ok[1]) out_raw[row[1]] = make_float4(p1[0], p1[1], p1[2], sig1);
        }
      }
    }
#undef RNERF_PE_KSTEP
#undef SLAB_PREFETCH
#undef SLAB_DONE
    tile = next_tile;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// T1 (MLP part): backward of the NerfMLP.  Replaces jax.value_and_grad through NerfMLP.__call__ (train.py:164 /
// rnerf/model_utils.py:30-90).
//   dgrad chain (this kernel): the same transposed-chain engine as the forward, with the weights transposed:
//       dX^T[k][row] = W[k][n] dY^T[n][row]   (A = W rows, B = dY in accumulator layout, bf16 hi/lo split -> 3 MFMAs)
//   dY_{l-1} = dX_l * 1[X_l > 0] uses the operands saved by the training forward as the ReLU mask (a saved operand is the
//   ReLU output; 0 <=> inactive).  Every dY_l (bf16 hi parts, the very B operands of the next dgrad layer) is written
//   slot-major for the wgrad kernel:  slot 16*l + s (l = 0..8), 144 + s (l = 9, 8 k-steps), 152 = head grads
//   (half 0: slot 0 = d raw_sigma, slots 1..3 = d raw_rgb).
// ------------------------------------------------------------------------------------------------------------------
constexpr int DY_L9 = 144, DY_HEADS = 152, DY_SLOTS = 153;
// dgrad MFMA passes per product: 22 = (W_hi + W_lo) * dY_hi, i.e. exact weights times bf16-rounded gradients — the same rounding the
// wgrad applies to dY anyway (measured worst gradient error 6.0e-3 of the tensor maximum; 3 passes: 5.1e-3 at +0.3 ms;
// 2 = (dY_hi + dY_lo) * W_hi: 6.8e-3 at the same speed)
constexpr int DGRAD_PASSES = 22;
// Internal dgrad variant of backward F16 (not an enum rnerf_backward value): ONE MFMA per product — the weights rounded to f16 like the
// gradients — selected when the FORWARD is the single-pass f16 one too.  The step is then one MFMA per product end to end (the arithmetic
// north_star names); behind the f16x3 forward the F16 backward keeps its exact (hi + lo) weights (passes 22): there the rounded weights
// would be the largest error left (gradient 4.9e-6 -> 4.1e-5 of max|g| from the default's on the bench batch), behind the f16 forward they
// change nothing measurable (9.2e-5 both ways) and take 0.19 ms off the dgrad (1.21 -> 1.03 ms; profiles/r05/README.md).
constexpr int kBwdF16OnePass = 3;
constexpr int kBwdBlocks = 8 * 8 + 8 * 16 * 8;   // (k-steps over n) x (8 input-feature tiles): L9 then L8..L1

// dgrad layer order: index 0 = MFMA layer 9 (Dense_10), 1 = layer 8 (Dense_9), 2..8 = layers 7..1 (Dense_7..Dense_1)
__host__ __device__ constexpr int bwd_dense(int i) { return i == 0 ? 10 : (i == 1 ? 9 : 9 - i); }
__host__ __device__ constexpr int bwd_blocks_before(int i) { return i == 0 ? 0 : 64 + (i - 1) * 128; }

template <int PREC>
__global__ void nerfmlp_pack_bwd_kernel(const float* __restrict__ params, char* __restrict__ packed) {
  using PP = Prec<PREC>;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= kBwdBlocks * 64) return;
  const int blk = gid >> 6, lane = gid & 63;
  int i = 0;
  while (i < 8 && blk >= bwd_blocks_before(i + 1)) ++i;
  const int rel = blk - bwd_blocks_before(i);
  const int s = rel / 8, kt = rel % 8;
  const int d = bwd_dense(i), out_dim = nerf_dense(d).out;
  const int kf = 32 * kt + (lane & 31), h = lane >> 5;        // input feature (row of the Dense kernel), < 256 always
  float w[8];
  for (int j = 0; j < 8; ++j) {
    const int n = prev_feature(s, h, j);
    w[j] = n < out_dim ? params[nerf_koff(d) + kf * out_dim + n] * PP::WSCALE : 0.f;
  }
  uint32_t hi[4], lo[4];
  for (int p = 0; p < 4; ++p) split2<PP::F16>(w[2 * p], w[2 * p + 1], hi[p], lo[p]);
  uint4* dst = (uint4*)(packed + (size_t)blk * PP::NP * 1024);
  dst[lane] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
  if (PP::NP == 2) dst[64 + lane] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

// dgrad twin of PrevConv: the B operands of k-step S of the NEXT dgrad GEMM = (state / WSCALE [+ d sigma * w_sigma]) * ReLU mask, split
// into 16-bit hi/lo parts, computed pair by pair in the shadow of the current k-step's MFMAs.
// SEAM: k-step 0 of a layer, converted by DgradSeam in the previous layer's last k-step.  Its d sigma term keeps the form k-step 0 has
// always had, fma(d sigma, w, state / WSCALE) — one rounding, where the steady k-steps round d sigma * w first — taken by a select.
template <int PREC, int S, bool NEED_LO, bool ONE = false, bool SEAM = false>
struct GradConv {
  using PP = Prec<PREC>;
  const f32x16& p0;   // m-tile 0 state (accumulator registers of the previous dgrad layer)
  float v1[8];        // m-tile 1 state (from LDS)
  float t0[8], t1[8]; // d raw_sigma * w_sigma of these 8 features for the two m-tiles (0 unless this layer receives d sigma)
  uint32_t w0, w1;    // mask word S>>2 of both m-tiles (all ones: no ReLU)
  uint32_t hi[2][4], lo[2][4];
  float x0, x1;
  bool wadd;          // SEAM: the layer receives d sigma (gw0 / gw1 of the two m-tiles) times the sigma weights wv of these 8 features
  float gw0, gw1, wv[8];
  __device__ __forceinline__ GradConv(const f32x16& p) : p0(p) {}
  template <int C, int PI>
  __device__ __forceinline__ void chunk() {
    constexpr int mt = PI >> 2, p = PI & 3;
    if constexpr (ONE && mt == 1) return;
    constexpr float INV_SCALE = 1.0f / PP::WSCALE;
    if constexpr (C == 0) {
      const float r0 = mt == 0 ? p0[8 * (S & 1) + 2 * p] : v1[2 * p];
      const float r1 = mt == 0 ? p0[8 * (S & 1) + 2 * p + 1] : v1[2 * p + 1];
      if constexpr (SEAM) {
        const float gw = mt == 0 ? gw0 : gw1;
        x0 = r0 * INV_SCALE; x1 = r1 * INV_SCALE;
        x0 = wadd ? fmaf(gw, wv[2 * p], x0) : x0;
        x1 = wadd ? fmaf(gw, wv[2 * p + 1], x1) : x1;
      } else {
        x0 = fmaf(r0, INV_SCALE, mt == 0 ? t0[2 * p] : t1[2 * p]);
        x1 = fmaf(r1, INV_SCALE, mt == 0 ? t0[2 * p + 1] : t1[2 * p + 1]);
      }
    } else if constexpr (C == 1) {
      const uint32_t w = mt == 0 ? w0 : w1;      // v_bfe_i32 spreads the flag into a 0 / ~0 word, v_and applies it: 2 ops per value
      constexpr int pos0 = 8 * (S & 3) + p, pos1 = pos0 + 4;
      uint32_t m0, m1;                           // (asm: hipcc rewrites the builtin form back into v_and + v_cmp + v_cndmask)
      asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m0) : "v"(w), "n"(pos0));
      asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m1) : "v"(w), "n"(pos1));
      x0 = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, x0) & m0);
      x1 = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, x1) & m1);
    } else if constexpr (C == 2) {
      hi[mt][p] = pack2<PP::F16>(x0, x1);
    } else if constexpr (C == 3) {
      if constexpr (NEED_LO) {
        float ha, hb;
        unpack2<PP::F16>(hi[mt][p], ha, hb);
        x0 -= ha; x1 -= hb;
      }
    } else {
      if constexpr (NEED_LO) lo[mt][p] = pack2<PP::F16>(x0, x1);
      else lo[mt][p] = 0;
    }
  }
  __device__ __forceinline__ KOpsT<ONE> result() const {
    KOpsT<ONE> o;
    o.h0 = make_uint4(hi[0][0], hi[0][1], hi[0][2], hi[0][3]); o.l0 = make_uint4(lo[0][0], lo[0][1], lo[0][2], lo[0][3]);
    if constexpr (ONE) { o.h1 = o.h0; o.l1 = o.l0; }
    else { o.h1 = make_uint4(hi[1][0], hi[1][1], hi[1][2], hi[1][3]); o.l1 = make_uint4(lo[1][0], lo[1][1], lo[1][2], lo[1][3]); }
    return o;
  }
};

// dgrad twin of SeamWork: the work of a dgrad layer's LAST k-step, in the shadow of its MFMAs.  Once the MFMAs of tile t are issued, tile
// t - 1 is final: in tile t's slots its m-tile 0 state moves to prev0[t - 1] and its m-tile 1 state to the wave's LDS state (both are dead
// by then: the last k-step's operands were converted a k-step earlier), and pair t - 1 of the NEXT layer's k-step 0 is converted from
// tile 0 (cv; its mask word was loaded a layer ahead, its sigma weights two k-steps ahead).  Tile 7 is handed over by finish().
template <int PREC, bool NEED_LO, bool ONE = false>
struct DgradSeam {
  f32x16 (&acc0)[8];
  f32x16 (&acc1)[8];
  f32x16 (&prev0)[8];
  float4* st1;
  GradConv<PREC, 0, NEED_LO, ONE, true> cv;      // pairs 0..3: m-tile 0 from acc0[0], pairs 4..7: m-tile 1 from acc1[0]
  __device__ __forceinline__ DgradSeam(f32x16 (&a0)[8], f32x16 (&a1)[8], f32x16 (&p0)[8], float4* s1) : acc0(a0), acc1(a1), prev0(p0), st1(s1), cv(a0[0]) {}
  template <int C, int T>
  __device__ __forceinline__ void move() {            // piece C of the hand-over of tile T
    if constexpr (C == 0) prev0[T] = acc0[T];
    else if constexpr (!ONE) st1[(T * 4 + C - 1) * 64] = make_float4(acc1[T][4 * (C - 1)], acc1[T][4 * (C - 1) + 1], acc1[T][4 * (C - 1) + 2], acc1[T][4 * (C - 1) + 3]);
  }
  template <int C, int Q>
  __device__ __forceinline__ void conv() {
    if constexpr (ONE && Q >= 4) return;
    if constexpr (C == 0 && Q >= 4) { cv.v1[2 * (Q & 3)] = acc1[0][2 * (Q & 3)]; cv.v1[2 * (Q & 3) + 1] = acc1[0][2 * (Q & 3) + 1]; }
    cv.template chunk<C, Q>();
  }
  template <int C, int PI>
  __device__ __forceinline__ void chunk() {
    if constexpr (PI >= 1) {
      move<C, PI - 1>();
      conv<C, PI - 1>();
      // pair 7 after pair 6 (GradConv keeps ONE pair in flight: x0 / x1)
      if constexpr (PI == 7 && C == 4) { conv<0, 7>(); conv<1, 7>(); conv<2, 7>(); conv<3, 7>(); conv<4, 7>(); }
    }
  }
  __device__ __forceinline__ void finish() {
    move<0, 7>(); move<1, 7>(); move<2, 7>(); move<3, 7>(); move<4, 7>();
  }
};

// Backward arithmetic (enum rnerf_backward): BF16 = gradients rounded to bf16 (8-bit significand), one 16-bit part per operand;
// F16 / F16X2 = every row's gradient chain is normalised by a power of two m_row >= max |d raw[row]| (the chain is linear in d raw, so
// the normalised values sit in f16's range whatever the loss scale), operands are f16 (11-bit significand) or f16 hi + lo (22 bits);
// the wgrad multiplies the saved activations by m_row / m_ref again (m_ref = max m_row, collected with an atomic).
template <int BWD> struct Bwd {
  static constexpr bool F16 = BWD != RNERF_BWD_BF16;
  static constexpr bool LO8 = BWD == RNERF_BWD_F16X3_LO8;                                 // the lo plane is stored as e4m3 bytes (lo8_pack)
  static constexpr int NP = (BWD == RNERF_BWD_F16X2 || LO8) ? 2 : 1;                      // parts stored per gradient / consumed per activation
  static constexpr int PREC = F16 ? RNERF_PREC_F16X3 : RNERF_PREC_BF16X3;                 // operand type + weight split of the dgrad MFMAs
  static constexpr int PASSES = (BWD == RNERF_BWD_F16X2 || LO8) ? 3 : (BWD == RNERF_BWD_F16 ? 22 : (BWD == kBwdF16OnePass ? 1 : DGRAD_PASSES));
  static constexpr bool NEED_LO = PASSES != 22 && PASSES != 1;
};
// dy buffer: uint4[DY_SLOTS * NP][R][2] operand planes (hi, then lo), then float row_scale[R] and uint32 m_ref bits (F16 modes)
__host__ __device__ constexpr size_t dy_plane_uint4(long long R, int np) { return (size_t)DY_SLOTS * np * (size_t)R * 2; }
__host__ __device__ constexpr size_t dy_addr(int q, long long t32, int m, int h) { return (((size_t)t32 * DY_SLOTS + q) * 32 + m) * 2 + h; }     // tile-major, see sv_addr

template <int BWD, bool ONE = false>
__global__ void __launch_bounds__(256, 1)
nerfmlp_dgrad_kernel(const char* __restrict__ packed_bwd, const float* __restrict__ fwd_aux, const uint4* __restrict__ saved,
                     long long save_rows, const float4* __restrict__ d_raw, long long total_rows, int n_tiles,
                     uint4* __restrict__ dy) {
  // ONE: 128-row tiles, one m-tile per wave (see nerfmlp_fwd_kernel); n_tiles then counts 128-row tiles
  using BW = Bwd<BWD>;
  using KOps = KOpsT<ONE>;
  constexpr int PREC = BW::PREC;
  constexpr int DGP = BW::PASSES;
  constexpr bool NEED_LO = BW::NEED_LO;
  using PP = Prec<PREC>;
  constexpr int SLAB = PP::SLAB;
  constexpr int WROWS = ONE ? 32 : 64, TROWS = 4 * WROWS;
  constexpr float INV_SCALE = 1.0f / PP::WSCALE;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 31, h = lane >> 5;
  float4* __restrict__ st1 = (float4*)(smem + 2 * SLAB + wave * 32768) + lane;
  int buf = 0;
  size_t off = 0;

  if ((int)blockIdx.x < n_tiles) { issue_slab<SLAB>(packed_bwd, 0u, wave, lane); off = SLAB; }
  slab_wait_dma();
  __syncthreads();

  float mref = 0.f;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const bool has_next_tile = tile + (int)gridDim.x < n_tiles;
    const long long srow0 = (long long)tile * TROWS + wave * WROWS + m;
    const long long t32_0 = (long long)tile * (TROWS / 32) + wave * (WROWS / 32);
    // An opaque per-tile copy of the aux base, as in the forward (auxt there): left alone, hipcc hoists the tile-invariant head and sigma
    // weight loads in front of the tile loop — 64 vectors loaded one by one, each waited for and spilled, and reloaded in every tile.
    const float* __restrict__ auxt = fwd_aux;
    asm volatile("" : "+s"(auxt));
    // rgb-head weights (Dense_11, [3][128]) of the 8 features this lane holds in each register group of n-tile t: 12 vectors per n-tile,
    // fetched as one batch — n-tile 0 here, beside the d raw read, n-tile t + 1 while n-tile t is formed
    const float* __restrict__ hw = auxt + AUX_WRGB + 4 * h;
    auto head_load = [&](int t, float4 (&W)[12]) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = 32 * t + 8 * q;
        W[3 * q] = gload4(hw + n); W[3 * q + 1] = gload4(hw + 128 + n); W[3 * q + 2] = gload4(hw + 256 + n);
      }
    };
    float4 Wc[12];
    head_load(0, Wc);
    float4 g[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      if (ONE && mt == 1) { g[1] = make_float4(0.f, 0.f, 0.f, 0.f); continue; }
      const long long row = srow0 + 32 * mt;
      g[mt] = row < total_rows ? d_raw[row] : make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (BW::F16) {          // row normalisation
        const float mx = fmaxf(fmaxf(fabsf(g[mt].x), fabsf(g[mt].y)), fmaxf(fabsf(g[mt].z), fabsf(g[mt].w)));
        const uint32_t ex = __builtin_bit_cast(uint32_t, mx) >> 23;
        // m_row = 2^(exponent(max |g|) - 5): 32 <= max |g / m_row| < 64 — 2^10 of headroom below f16's 65504 for growth along the chain,
        // and every value above 0.2 % of the row's maximum keeps a NORMAL f16 lo part.  Rows with no (or a subnormal) gradient
        // contribute nothing: m_row = 0 (a non-finite d raw still yields NaN gradients: NaN * 0).
        const bool okx = ex >= 8 && ex <= 250;
        const float m_row = okx ? __builtin_bit_cast(float, (ex - 5) << 23) : 0.0f;
        const float inv = okx ? __builtin_bit_cast(float, (259 - ex) << 23) : 0.0f;
        g[mt].x *= inv; g[mt].y *= inv; g[mt].z *= inv; g[mt].w *= inv;
        float* rs = (float*)(dy + dy_plane_uint4(save_rows, BW::NP));
        if (h == 0) rs[row] = m_row;
        mref = fmaxf(mref, m_row);
      }
    }
    f32x16 acc0[8], acc1[8], prev0[8];
    float4 wna = make_float4(0.f, 0.f, 0.f, 0.f), wnb = wna, wk0a = wna, wk0b = wna;      // sigma weights in flight, see RNERF_DG_KSTEP
    KOps cur;                                   // operands of the next k-step; across a layer seam: k-step 0 of the next layer (DgradSeam)

    auto dy_store = [&](int q, const KOps& o) {
      uint4* dst = dy + dy_addr(q, t32_0, m, h);
      stream_store(dst, o.h0);
      if constexpr (!ONE) stream_store(dst + (size_t)DY_SLOTS * 64, o.h1);
      if constexpr (BW::LO8) {
        uint2* dl = (uint2*)(dy + dy_plane_uint4(save_rows, 1)) + dy_addr(q, t32_0, m, h);
        stream_store8(dl, lo8_pack<true>(o.l0, LO8_SCALE_D));
        if constexpr (!ONE) stream_store8(dl + (size_t)DY_SLOTS * 64, lo8_pack<true>(o.l1, LO8_SCALE_D));
      } else if constexpr (BW::NP == 2) {
        uint4* dl = dst + dy_plane_uint4(save_rows, 1);
        stream_store(dl, o.l0);
        if constexpr (!ONE) stream_store(dl + (size_t)DY_SLOTS * 64, o.l1);
      }
    };
    // ReLU masks: one uint4 of non-zero flags per (row, half) per layer (SAVE_MASK), fetched one layer ahead
    auto mask_at = [&](int set, uint4& a, uint4& b) {
      const uint32_t* src = (const uint32_t*)(saved + sv_mask0(save_rows)) + sv_mask_addr(set * 4, t32_0, m, h);
      constexpr size_t ws = 64, mt1 = 36 * 64;          // next mask word of the set / the wave's second 32-row tile
#define RNERF_NTL(P) __builtin_nontemporal_load(P)
      a = make_uint4(RNERF_NTL(src), RNERF_NTL(src + ws), RNERF_NTL(src + 2 * ws), RNERF_NTL(src + 3 * ws));
      if constexpr (ONE) b = make_uint4(0, 0, 0, 0);
      else b = make_uint4(RNERF_NTL(src + mt1), RNERF_NTL(src + ws + mt1), RNERF_NTL(src + 2 * ws + mt1), RNERF_NTL(src + 3 * ws + mt1));
#undef RNERF_NTL
    };
    // operands of k-step s from the state (prev0 / st1): x = (state + dsig * wadd) * 1[mask != 0]
    // (wadd: add d sigma * w_sigma, the 8 sigma weights of this lane's features given in wa / wb)
    auto grad_ops = [&](int s, bool use_mask, const uint4 mk0, const uint4 mk1, bool wadd, const float4 wa, const float4 wb) -> KOps {
      const float wv[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
      float r1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if constexpr (!ONE) {
        const float4 u0 = st1[((s >> 1) * 4 + 2 * (s & 1)) * 64], u1 = st1[((s >> 1) * 4 + 2 * (s & 1) + 1) * 64];
        r1[0] = u0.x; r1[1] = u0.y; r1[2] = u0.z; r1[3] = u0.w; r1[4] = u1.x; r1[5] = u1.y; r1[6] = u1.z; r1[7] = u1.w;
      }
      const uint32_t w0 = (s >> 2) == 0 ? mk0.x : ((s >> 2) == 1 ? mk0.y : ((s >> 2) == 2 ? mk0.z : mk0.w));
      const uint32_t w1 = (s >> 2) == 0 ? mk1.x : ((s >> 2) == 1 ? mk1.y : ((s >> 2) == 2 ? mk1.z : mk1.w));
      float x0[8], x1[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float a = prev0[s >> 1][8 * (s & 1) + j] * INV_SCALE, b = r1[j] * INV_SCALE;
        if (wadd) { const float w = wv[j]; a = fmaf(g[0].w, w, a); b = fmaf(g[1].w, w, b); }
        if (use_mask) {
          const uint32_t bit = 1u << (8 * (s & 3) + (j >> 1) + 4 * (j & 1));
          a = (w0 & bit) ? a : 0.f;
          b = (w1 & bit) ? b : 0.f;
        }
        x0[j] = a; x1[j] = b;
      }
      KOps o;
      if constexpr (ONE) { split8<PREC>(x0, o.h0, o.l0); if constexpr (!(NEED_LO || BW::NP == 2)) o.l0 = make_uint4(0, 0, 0, 0); o.h1 = o.h0; o.l1 = o.l0; }
      else if constexpr (NEED_LO || BW::NP == 2) { split8<PREC>(x0, o.h0, o.l0); split8<PREC>(x1, o.h1, o.l1); }
      else {
        o.h0 = make_uint4(pack2<PP::F16>(x0[0], x0[1]), pack2<PP::F16>(x0[2], x0[3]), pack2<PP::F16>(x0[4], x0[5]), pack2<PP::F16>(x0[6], x0[7]));
        o.h1 = make_uint4(pack2<PP::F16>(x1[0], x1[1]), pack2<PP::F16>(x1[2], x1[3]), pack2<PP::F16>(x1[4], x1[5]), pack2<PP::F16>(x1[6], x1[7]));
        o.l0 = make_uint4(0, 0, 0, 0); o.l1 = o.l0;
      }
      return o;
    };
    auto layer_end = [&]() {
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        prev0[t] = acc0[t];
        if constexpr (!ONE) {
#pragma unroll
          for (int rq = 0; rq < 4; ++rq)
            st1[(t * 4 + rq) * 64] = make_float4(acc1[t][4 * rq], acc1[t][4 * rq + 1], acc1[t][4 * rq + 2], acc1[t][4 * rq + 3]);
        }
      }
    };
#define SLAB_PREFETCH(DO_NEXT)                                                                                       \
  do { if (DO_NEXT) { issue_slab<SLAB>(packed_bwd + off, (unsigned)((buf ^ 1) * SLAB), wave, lane); off += SLAB; } } while (0)
#define SLAB_DONE() do { slab_wait_dma(); __syncthreads(); buf ^= 1; } while (0)

    // ---- head gradients: record them for the wgrad kernel, push d raw_rgb through the rgb head (Dense_11) into the state
    {
      KOps o;
      float hz0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, hz1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (h == 0) { hz0[0] = g[0].w; hz0[1] = g[0].x; hz0[2] = g[0].y; hz0[3] = g[0].z; hz1[0] = g[1].w; hz1[1] = g[1].x; hz1[2] = g[1].y; hz1[3] = g[1].z; }
      split8<PREC>(hz0, o.h0, o.l0);
      if constexpr (ONE) { o.h1 = o.h0; o.l1 = o.l0; } else split8<PREC>(hz1, o.h1, o.l1);
      dy_store(DY_HEADS, o);
#pragma unroll
      for (int t = 0; t < 4; ++t) {       // register r of n-tile t is feature n = 32 t + 8 (r >> 2) + 4 h + (r & 3)
        float4 Wn[12];
        if (t + 1 < 4) head_load(t + 1, Wn);
        RNERF_PIN();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 vr = Wc[3 * q], vg = Wc[3 * q + 1], vb = Wc[3 * q + 2];
          const float wrv[4] = {vr.x, vr.y, vr.z, vr.w}, wgv[4] = {vg.x, vg.y, vg.z, vg.w}, wbv[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float wr = wrv[i], wg = wgv[i], wb = wbv[i];
            acc0[t][4 * q + i] = (g[0].x * wr + g[0].y * wg + g[0].z * wb) * PP::WSCALE;       // the state is kept in the accumulators' units (x WSCALE)
            if constexpr (!ONE) acc1[t][4 * q + i] = (g[1].x * wr + g[1].y * wg + g[1].z * wb) * PP::WSCALE;
          }
        }
        if (t + 1 < 4) {
#pragma unroll
          for (int q = 0; q < 12; ++q) Wc[q] = Wn[q];
        }
      }
#pragma unroll
      for (int t = 4; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          acc0[t][r] = 0.f;
          if constexpr (!ONE) acc1[t][r] = 0.f;
        }
      layer_end();
    }

    // ---- dgrad of MFMA layer 9 (Dense_10): k-steps over its 128 outputs; state masked by the saved rgb-head input
    {
      uint4 ma, mb;
      mask_at(8, ma, mb);
      cur = grad_ops(0, true, ma, mb, false, wk0a, wk0b);
      // sigma weights: the two vectors of k-step S + 2 are fetched in k-step S (the k-step's closing wait covers them), whether the layer
      // takes d sigma or not (wl: the sigma weights for layer 7, else the aux zeros; wl_next: the same for the layer after this one) —
      // wna / wnb hold those of k-step S + 1, wk0a / wk0b those of the next layer's k-step 0
#define RNERF_DG_KSTEP(S, NSTEPS, SLOT0, PREFETCH_STMT)                                                                       \
      {                                                                                                                         \
        dy_store((SLOT0) + S, cur);                                                                                             \
        const float* __restrict__ wsrc = (S + 2 < NSTEPS) ? wl + 16 * (S + 2) : wl_next + 16 * (S + 2 - NSTEPS);                \
        const float4 wfa = gload4(wsrc), wfb = gload4(wsrc + 8);                                                                \
        auto dma = [&]() { PREFETCH_STMT; };   /* issued after the first two tiles' MFMAs (an LDS-DMA instruction costs ~100 issue cycles) */ \
        if constexpr (S + 1 < NSTEPS) {                                                                                         \
          GradConv<PREC, S + 1, NEED_LO, ONE> cv(prev0[(S + 1) >> 1]);                                                                   \
          if constexpr (!ONE) {                                                                                                 \
            const float4 u0 = st1[(((S + 1) >> 1) * 4 + 2 * ((S + 1) & 1)) * 64], u1 = st1[(((S + 1) >> 1) * 4 + 2 * ((S + 1) & 1) + 1) * 64]; \
            cv.v1[0] = u0.x; cv.v1[1] = u0.y; cv.v1[2] = u0.z; cv.v1[3] = u0.w; cv.v1[4] = u1.x; cv.v1[5] = u1.y; cv.v1[6] = u1.z; cv.v1[7] = u1.w; \
          }                                                                                                                     \
          if (wadd) {   /* ONE test per k-step (per value it was 8 branches); only layer 7 takes it */                          \
            const float wv[8] = {wna.x, wna.y, wna.z, wna.w, wnb.x, wnb.y, wnb.z, wnb.w};                                       \
            _Pragma("unroll") for (int j = 0; j < 8; ++j) { cv.t0[j] = g[0].w * wv[j]; cv.t1[j] = g[1].w * wv[j]; }             \
          } else {                                                                                                              \
            _Pragma("unroll") for (int j = 0; j < 8; ++j) { cv.t0[j] = 0.f; cv.t1[j] = 0.f; }                                   \
          }                                                                                                                     \
          cv.w0 = ((S + 1) >> 2) == 0 ? ma.x : (((S + 1) >> 2) == 1 ? ma.y : (((S + 1) >> 2) == 2 ? ma.z : ma.w));             \
          cv.w1 = ((S + 1) >> 2) == 0 ? mb.x : (((S + 1) >> 2) == 1 ? mb.y : (((S + 1) >> 2) == 2 ? mb.z : mb.w));             \
          kstep_mfma<PREC, 8, 0, S == 0, GradConv<PREC, S + 1, NEED_LO, ONE>, decltype(dma), DGP>(acc0, acc1, cur, smem + buf * SLAB, lane, cv, dma); \
          cur = cv.result();                                                                                                    \
        } else {   /* the layer seam: hand the state over and convert the next layer's k-step 0 (seam_w0 / seam_w1: its mask words) */  \
          DgradSeam<PREC, NEED_LO, ONE> seam(acc0, acc1, prev0, st1);                                                           \
          seam.cv.w0 = seam_w0; seam.cv.w1 = seam_w1; seam.cv.wadd = seam_wadd; seam.cv.gw0 = g[0].w; seam.cv.gw1 = g[1].w;     \
          seam.cv.wv[0] = wk0a.x; seam.cv.wv[1] = wk0a.y; seam.cv.wv[2] = wk0a.z; seam.cv.wv[3] = wk0a.w;                       \
          seam.cv.wv[4] = wk0b.x; seam.cv.wv[5] = wk0b.y; seam.cv.wv[6] = wk0b.z; seam.cv.wv[7] = wk0b.w;                       \
          kstep_mfma<PREC, 8, 0, false, DgradSeam<PREC, NEED_LO, ONE>, decltype(dma), DGP>(acc0, acc1, cur, smem + buf * SLAB, lane, seam, dma); \
          seam.finish();                                                                                                        \
          cur = seam.cv.result();                                                                                               \
        }                                                                                                                       \
        if constexpr (S + 2 == NSTEPS) { wk0a = wfa; wk0b = wfb; } else { wna = wfa; wnb = wfb; }                               \
        SLAB_DONE();                                                                                                            \
      }
      {
        constexpr bool wadd = false, seam_wadd = false;
        constexpr uint32_t seam_w0 = ~0u, seam_w1 = ~0u;      // layer 8, the bottleneck, has no ReLU
        const float* __restrict__ wl = auxt + AUX_ZERO + 4 * h;
        const float* __restrict__ wl_next = wl;
        RNERF_DG_KSTEP(0, 8, DY_L9, SLAB_PREFETCH(true)) RNERF_DG_KSTEP(1, 8, DY_L9, SLAB_PREFETCH(true))
        RNERF_DG_KSTEP(2, 8, DY_L9, SLAB_PREFETCH(true)) RNERF_DG_KSTEP(3, 8, DY_L9, SLAB_PREFETCH(true))
        RNERF_DG_KSTEP(4, 8, DY_L9, SLAB_PREFETCH(true)) RNERF_DG_KSTEP(5, 8, DY_L9, SLAB_PREFETCH(true))
        RNERF_DG_KSTEP(6, 8, DY_L9, SLAB_PREFETCH(true)) RNERF_DG_KSTEP(7, 8, DY_L9, SLAB_PREFETCH(true))
      }
    }

    // ---- dgrad of MFMA layers 8..1: dY_l = (dX_{l+1} [+ d sigma * w_sigma for l = 7]) * 1[X_{l+1} > 0]  (no mask for the bottleneck l = 8)
    uint4 nma = make_uint4(0, 0, 0, 0), nmb = nma;      // mask of the NEXT iteration (set l-1), loaded a whole layer ahead
#pragma unroll 1
    for (int l = 8; l >= 1; --l) {
      const bool use_mask = l != 8;
      const bool wadd = l == 7;
      const float* __restrict__ wl = auxt + (l == 7 ? AUX_WSIG : AUX_ZERO) + 4 * h;
      const float* __restrict__ wl_next = auxt + (l == 8 ? AUX_WSIG : AUX_ZERO) + 4 * h;
      uint4 ma = nma, mb = nmb;                  // set l = the ReLU mask of the input of layer l+1
      if (!use_mask) { ma = make_uint4(~0u, ~0u, ~0u, ~0u); mb = ma; }
      mask_at(l - 1, nma, nmb);
      const bool seam_wadd = l == 8;             // the seam converts k-step 0 of layer l - 1 (l = 1: of the dY_0 record)
      const uint32_t &seam_w0 = nma.x, &seam_w1 = nmb.x;
      const int slot0 = 16 * l;
#define RNERF_DG_PF(S) do { if ((S) == 15 && l == 1) { if (has_next_tile) off = 0; SLAB_PREFETCH(has_next_tile); } else SLAB_PREFETCH(true); } while (0)
      RNERF_DG_KSTEP(0, 16, slot0, RNERF_DG_PF(0)) RNERF_DG_KSTEP(1, 16, slot0, RNERF_DG_PF(1)) RNERF_DG_KSTEP(2, 16, slot0, RNERF_DG_PF(2))
      RNERF_DG_KSTEP(3, 16, slot0, RNERF_DG_PF(3)) RNERF_DG_KSTEP(4, 16, slot0, RNERF_DG_PF(4)) RNERF_DG_KSTEP(5, 16, slot0, RNERF_DG_PF(5))
      RNERF_DG_KSTEP(6, 16, slot0, RNERF_DG_PF(6)) RNERF_DG_KSTEP(7, 16, slot0, RNERF_DG_PF(7)) RNERF_DG_KSTEP(8, 16, slot0, RNERF_DG_PF(8))
      RNERF_DG_KSTEP(9, 16, slot0, RNERF_DG_PF(9)) RNERF_DG_KSTEP(10, 16, slot0, RNERF_DG_PF(10)) RNERF_DG_KSTEP(11, 16, slot0, RNERF_DG_PF(11))
      RNERF_DG_KSTEP(12, 16, slot0, RNERF_DG_PF(12)) RNERF_DG_KSTEP(13, 16, slot0, RNERF_DG_PF(13)) RNERF_DG_KSTEP(14, 16, slot0, RNERF_DG_PF(14))
      RNERF_DG_KSTEP(15, 16, slot0, RNERF_DG_PF(15))
#undef RNERF_DG_PF
    }
#undef RNERF_DG_KSTEP

    // ---- dY_0 = dX_1 * 1[X_1 > 0]: only recorded (layer 0's inputs are constants); k-step 0 comes from Dense_1's seam
    dy_store(0, cur);
#pragma unroll
    for (int s = 1; s < 16; ++s) {
      const KOps o = grad_ops(s, true, nma, nmb, false, wk0a, wk0b);
      dy_store(s, o);
    }
#undef SLAB_PREFETCH
#undef SLAB_DONE
  }
  if constexpr (BW::F16) {      // m_ref = max m_row over all rows (positive floats order like their bit patterns)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mref = fmaxf(mref, __shfl_xor(mref, o));
    if (lane == 0 && mref > 0.f)
      atomicMax((unsigned int*)((float*)(dy + dy_plane_uint4(save_rows, BW::NP)) + save_rows), __builtin_bit_cast(unsigned int, mref));
  }
}

// ------------------------------------------------------------------------------------------------------------------
// wgrad: dW[k][n] = sum_rows X[row][k] * dY[row][n] for one (X slots, dY slots) job.  The saved tensors hold, per lane, 8
// FEATURES of one ROW (the forward's B-operand layout); an MFMA contracts over the 8 values a lane holds, so both operands
// must first be transposed to "lane = feature, slots = rows".  The transposition is itself done on the matrix cores:
//     D = X_frag(k-step 2t) * I_lo + X_frag(k-step 2t+1) * I_hi        (A = the saved operand, B = a shifted identity)
// puts feature 16a + 8h + j of the two k-steps in output LANE 16a+8h+j and the wave's 32 rows in the 16 accumulator
// registers (exact: one non-zero product per output) -> repacked to bf16 they are wgrad operands.  Each wave transposes
// its own 32 rows, publishes the fragments in LDS, and after a barrier accumulates its share of the dW tiles over the 128
// rows of the workgroup.  Partials per workgroup are summed (and the slot permutation undone) by wgrad_reduce_kernel.
// ------------------------------------------------------------------------------------------------------------------
template <bool F16>
__device__ __forceinline__ uint4 shifted_identity(int lane, int a) {   // B operand: 1 at slot (h, j) of column 16a + 8h + j
  const int col = lane & 31, h = lane >> 5;
  uint32_t w[4] = {0, 0, 0, 0};
  if ((col >> 4) == a && ((col >> 3) & 1) == h) { const int j = col & 7; w[j >> 1] = (F16 ? 0x3C00u : 0x3F80u) << (16 * (j & 1)); }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ void pack_rows_bf16(const f32x16& d, uint4& u0, uint4& u1) {
  u0 = make_uint4(pack2<false>(d[0], d[1]), pack2<false>(d[2], d[3]), pack2<false>(d[4], d[5]), pack2<false>(d[6], d[7]));
  u1 = make_uint4(pack2<false>(d[8], d[9]), pack2<false>(d[10], d[11]), pack2<false>(d[12], d[13]), pack2<false>(d[14], d[15]));
}

// job description for the reduction: where the slot-ordered partial rows/columns land in the flat fp32 gradient buffer
struct WgradJob {
  int dense;      // Dense_k index in the flat parameter buffer
  int xkind;      // 0 = position encoding slots, 1 = previous-layer slots, 2 = view encoding slots
  int row_off;    // kernel row offset of this X block (256 for the concat parts)
  int dkind;      // 0 = layer outputs (prev_feature order), 1 = sigma head (slot 0 of the head grads), 2 = rgb head (slots 1..3)
  int KT, NT, write_bias;
  // merged jobs of the transpose-read kernel (an operand stream that two Dense blocks share is read once): the k-tiles from KTa on are
  // a second X segment (xkind2 / row_off2: the concat rows of the same Dense), the n-tiles from NTa on a second dY segment (dense2 /
  // dkind2: the sigma head beside Dense_9).  Single-segment jobs have KTa = KT, NTa = NT.
  int KTa, xkind2, row_off2, NTa, dense2, dkind2;
  int bias_sigma;  // rgb-head job: column 0 of its bias row is the sigma head's bias gradient (Dense_8), written from here
};
// all jobs of one NerfMLP in ONE launch: workgroups [wg0[j], wg0[j+1]) belong to job j
struct WgradTable {
  int n;
  int qx[16], KSx[16], qd[16], KSd[16], wg0[17];
  int qx2[16], qd2[16], KSd2[16];         // slot bases of the second segments, k-steps of the second dY segment
  long long poff[16], pboff[16];          // float offsets of the job's partial blocks in the workspace
  WgradJob job[16];
};

// One job shape (KT k-tiles of X, KSd k-steps = ceil(KSd/2) n-tiles of dY) is a compile-time instance: with run-time shapes the
// compiler guards every load with a branch and a vmcnt(0), which serialises the 32 loads of a chunk (measured: 21 us per chunk).
// Workgroup = 8 waves = 2 per SIMD (<= 256 registers each): waves 0..3 fetch + transpose the X slots of row groups 0..3, waves
// 4..7 the dY slots; in the accumulate phase wave w owns k-tile w (all n-tiles).  One wave's load waits / packing VALU overlap the
// partner wave's MFMAs, and the prefetch registers per wave halve (the 4-wave form with 2 k-tiles per wave took 1.92 ms, this 1.42).
template <bool X_F16, int KT, int KSd>
__device__ __forceinline__ void wgrad_body(const uint4* __restrict__ saved, const uint4* __restrict__ dy, long long R, long long total_rows,
                                            int n_chunks, float* __restrict__ pg, float* __restrict__ pbias, int qx, int qd, int g, int G,
                                            char* smem) {
  constexpr int NT = (KSd + 1) / 2;
  constexpr int NOP = 2 * (KT > NT ? KT : NT);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2, rw = wave & 3;
  const int m = lane & 31, h = lane >> 5;
  uint4* myT = (uint4*)(smem + rw * 32768) + lane + (grp ? 16 * 64 : 0);   // slot*64: X^T fragments 0..15, dY^T fragments 16..31
  const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const uint4 il = grp ? shifted_identity<false>(lane, 0) : shifted_identity<X_F16>(lane, 0);
  const uint4 ih = grp ? shifted_identity<false>(lane, 1) : shifted_identity<X_F16>(lane, 1);
  const uint32_t one2 = (m == 0) ? 0x3F803F80u : 0u;
  const uint4 ones = make_uint4(one2, one2, one2, one2);
  const uint4 z4 = make_uint4(0, 0, 0, 0);
  f32x16 acc[NT], accb = zero;
#pragma unroll
  for (int b = 0; b < NT; ++b) acc[b] = zero;
  uint4 opr[NOP];
  auto load_chunk = [&](int chunk) {
    const long long t32 = (long long)chunk * 4 + rw;
    if (grp == 0) {
      const uint4* base = saved + sv_addr(qx, t32, m, h);
#pragma unroll
      for (int t = 0; t < 2 * KT; ++t) opr[t] = stream_load(base + t * 64);
    } else {
      const uint4* base = dy + dy_addr(qd, t32, m, h);
#pragma unroll
      for (int t = 0; t < 2 * NT; ++t) opr[t] = t < KSd ? stream_load(base + t * 64) : z4;
    }
  };
  if (g < n_chunks) load_chunk(g);
  for (int chunk = g; chunk < n_chunks; chunk += G) {
    const bool ok = (long long)chunk * 128 + rw * 32 + m < total_rows;
    if (grp == 0) {
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        f32x16 d = mfma16<X_F16>(opr[2 * t], il, zero);
        d = mfma16<X_F16>(opr[2 * t + 1], ih, d);
        uint4 u0, u1;
        pack_rows_bf16(d, u0, u1);
        myT[(2 * t) * 64] = u0; myT[(2 * t + 1) * 64] = u1;
      }
    } else {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const uint4 a0 = ok ? opr[2 * t] : z4, a1 = ok ? opr[2 * t + 1] : z4;   // padded rows carry replayed data: they must not contribute
        f32x16 d = mfma16<false>(a0, il, zero);
        d = mfma16<false>(a1, ih, d);
        uint4 u0, u1;
        pack_rows_bf16(d, u0, u1);
        myT[(2 * t) * 64] = u0; myT[(2 * t + 1) * 64] = u1;
      }
    }
    __syncthreads();
    if (chunk + G < n_chunks) load_chunk(chunk + G);
    if (wave < KT || wave < NT) {
#pragma unroll 1
      for (int v = 0; v < 4; ++v) {
        const uint4* T = (const uint4*)(smem + v * 32768) + lane;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          if (wave < KT) {
            const uint4 a = T[(2 * wave + u) * 64];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = mfma16<false>(a, T[(16 + 2 * nt + u) * 64], acc[nt]);
          }
          if (wave < NT) accb = mfma16<false>(ones, T[(16 + 2 * wave + u) * 64], accb);
        }
      }
    }
    __syncthreads();
  }
  constexpr size_t ldn = (size_t)NT * 32;
  if (wave < KT) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = (r & 3) + 8 * (r >> 2) + 4 * h;
        pg[(size_t)(wave * 32 + i) * ldn + nt * 32 + m] = acc[nt][r];
      }
    }
  }
  if (wave < NT && h == 0) pbias[wave * 32 + m] = accb[0];
}

// ---- wgrad of the row-normalised f16 modes (RNERF_BWD_F16: NP = 1, RNERF_BWD_F16X2: NP = 2): no transposition phase ------------------------
// The saved tensors are row-major per slot ([row][half][8 features] = 32 B per row); an MFMA operand wants, per lane, 8 ROWS of one
// feature.  gfx950's LDS transpose read (ds_read_b64_tr_b16: within a 16-lane group, destination lane i, element j receives element
// (i & 3) of the 8 bytes addressed by source lane 4 j + (i >> 2); probed by tools/ubench/tr_read.hip) does that on the way out of LDS, so
//   * the operand slots travel HBM -> LDS by DMA (global_load_lds_dwordx4, no registers), 16 rows (one MFMA k-step) at a time, through a
//     ring of 4 (hi + lo) or 8 steps: all but one in flight while one is consumed — the kernel is paced by HBM (intensity 192 flop/B in the hi + lo mode);
//   * one DMA instruction builds one 1 KiB "block" = 16 rows x 32 features (two slots: a k-tile of X or an n-tile of dY) as
//     [row r][slot parity a][32 B]: lane L = 4 r + 2 a + h fetches the 16 B (slot 2 t + a, row r, half h).  A transpose read of a
//     32-lane half then covers 256 contiguous bytes: conflict-free;
//   * A operand of k-tile t: lane (m = l & 31, kh = l >> 5) reads rows 8 kh .. 8 kh + 7 of feature position m (= 16 a + p, p the position in
//     the slot's row — the order wgrad_reduce_kernel already undoes) with two transpose reads; B operands of dY the same way;
//   * the per-row scale m_row / m_ref (a power of two <= 1) multiplies the X operands as packed f16 (exact above the subnormal range; rows
//     that far below the largest carry nothing, as before); the bias row sum_rows m_row dY^[row][n] is an MFMA whose A operand holds the
//     scales in row m = 0;
//   * 8 waves = WK x WN, each accumulating TK x TN output tiles over all rows of its workgroup: per k-step TK + TN operand fetches feed
//     TK TN MFMAs (x 3 in the hi + lo mode).
// (Round 2's first form transposed on the matrix cores like wgrad_body below, through registers and LDS writes: 3.5 ms for the hi + lo
// mode on the bench workload against 2.2 ms for this one, which runs at ~5.2 TB/s of operand stream.)
// NT == 9 (Dense_9 + the sigma head): the 8 x 8 split, and the ninth n-tile as ONE extra tile per wave (k-tile 2 wk + wn, one of its own)
template <int KT, int NT> struct WgTrShape {
  static constexpr int EXTRA = NT == 9 ? 1 : 0, NTR = NT - EXTRA;
  static constexpr int WK = KT == 10 ? 2 : (KT == 9 ? 3 : (KT >= 8 ? (NTR >= 4 ? 4 : 8) : (KT >= 4 ? 4 : KT)));
  static constexpr int WN = (8 / WK) < NTR ? (8 / WK) : NTR;
  static constexpr int TK = KT / WK, TN = NTR / WN;
  static_assert(WK * TK == KT && WN * TN == NTR && WK * WN <= 8 && (!EXTRA || (TK == 2 && WN == 2)), "tile split");
};
constexpr int WGTR_NCH = 2;      // n-tiles of B fragments fetched at a time when the A side is resident

__device__ __forceinline__ half8 tr_read8(const char* p) {      // rows k .. k+3 at p, rows k+4 .. k+7 at p + 256 (4 rows x 64 B)
  typedef short short4v __attribute__((ext_vector_type(4)));
  typedef short short8v __attribute__((ext_vector_type(8)));
  typedef __attribute__((address_space(3))) short4v lds_short4;
  const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4*)p);
  const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4*)(p + 256));
  return __builtin_bit_cast(half8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}
__device__ __forceinline__ f32x16 mfma_h8(const half8 a, const half8 b, const f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
template <int N> __device__ __forceinline__ void wait_vmcnt() {
  __builtin_amdgcn_s_waitcnt(0x0F70 | (N & 15) | ((N >> 4) << 14));
  asm volatile("" ::: "memory");
}

struct WgTrSegs { int qx, KTa, qx2, qd, NTa, KSd, qd2, KSd2; };    // slot bases / extents of the (up to two) X and dY segments of a job
// the slot pair (block parity a = 0 / 1) of X k-tile t / of dY n-tile nt
__device__ __forceinline__ void x_slots(const WgTrSegs& sg, int t, int& s0, int& s1) {
  s0 = t < sg.KTa ? sg.qx + 2 * t : sg.qx2 + 2 * (t - sg.KTa);
  s1 = s0 + 1;
}
__device__ __forceinline__ void d_slots(const WgTrSegs& sg, int nt, int& s0, int& s1) {
  const int rel = nt < sg.NTa ? 2 * nt : 2 * (nt - sg.NTa);
  const int qb = nt < sg.NTa ? sg.qd : sg.qd2, ks = nt < sg.NTa ? sg.KSd : sg.KSd2;
  s0 = qb + (rel < ks ? rel : ks - 1);      // a slot beyond the segment's k-steps repeats its last one: those columns are dropped by the reduction
  s1 = qb + (rel + 1 < ks ? rel + 1 : ks - 1);
}

// One DMA instruction's source, per ring step: (wave-uniform base of its slot pair and plane, advanced by a uniform stride per 32-row tile
// and per 16-row half of it: SGPRs) + (lane part: one 32-bit VGPR per block)
struct WgTrDma { const char* sbase; unsigned voff, tstride, hstride; };
// lane part of every 16-bit transpose-read address: row (8 kh + (i >> 2)) * 64 + slot parity a * 32 + (i & 3) * 8, i = lane & 15
__device__ __forceinline__ unsigned wgtr_lane_off(int lane) {
  return (unsigned)((8 * (lane >> 5) + ((lane & 15) >> 2)) * 64 + ((lane >> 4) & 1) * 32 + (lane & 3) * 8);
}
constexpr int wgtr_step_bytes(int nblk) { return (nblk + 1) * 1024; }      // the blocks of a ring step + the row-scale block (64 B used)

// ---- what differs between the operand formats of the transposing wgrad: the blocks of a ring step and how fragments come out of them ------
// A policy names the planes (LO: lo planes beside the hi ones; NPLANES: dY planes ahead of the row scales), the ring (NBUF steps of
// nblk(KT, NT) blocks; lds_bytes() for the largest job: 10 k-tiles + 8 n-tiles), what the DMA instruction of block b fetches (dma) and
// from where at local step sc of 32-row tile t32 (step_src), and the fragment reads out of the ring slot at ring0 (Frags: read_a gives
// k-tile t of X times the row scales, read_b n-tile nt of dY; the hi part, and the lo part where LO).
// f16 planes (RNERF_BWD_F16: NP = 1, RNERF_BWD_F16X2: NP = 2): block (NP t + part) is plane `part` of tile t
template <int NP> struct F16Planes {
  static constexpr bool LO = NP == 2;
  static constexpr int NPLANES = NP;
  static constexpr int NBUF = NP == 2 ? 4 : 8;       // ring depth: what fits 160 KiB
  static constexpr int nblk(int KT, int NT) { return (KT + NT) * NP; }
  static constexpr int lds_bytes() { return NBUF * wgtr_step_bytes(nblk(10, 8)); }
  template <int KT, int NT>
  static __device__ __forceinline__ WgTrDma dma(int b, int lane, const uint4* __restrict__ saved, const uint4* __restrict__ dy, long long R, const WgTrSegs& sg) {
    // lane L = 4 r + 2 a + h fetches the 16 B (slot a of the pair, row r, half h)
    const int r = lane >> 2, a = (lane >> 1) & 1, h = lane & 1;
    const int t = b / NP, part = b % NP;
    int slot0, slot1;
    const uint4* base;
    WgTrDma d;
    if (t < KT) {
      x_slots(sg, t, slot0, slot1);
      base = saved + (part ? sv_lo0(R) : 0);
      d.tstride = (unsigned)(SAVE_SLOTS * 64 * sizeof(uint4));
    } else {
      d_slots(sg, t - KT, slot0, slot1);
      base = dy + (part ? dy_plane_uint4(R, 1) : 0);
      d.tstride = (unsigned)(DY_SLOTS * 64 * sizeof(uint4));
    }
    static_assert(sv_addr(1, 0, 0, 0) == dy_addr(1, 0, 0, 0) && sv_addr(0, 0, 1, 1) == dy_addr(0, 0, 1, 1), "one lane-offset formula for both tensors");
    d.sbase = (const char*)(base + sv_addr(__builtin_amdgcn_readfirstlane(slot0), 0, 0, 0));
    d.voff = (unsigned)((sv_addr(a ? __builtin_amdgcn_readfirstlane(slot1 - slot0) : 0, 0, r, h)) * sizeof(uint4));
    d.hstride = 0;      // one constant for every f16 block: in step_src
    return d;
  }
  static __device__ __forceinline__ const char* step_src(const WgTrDma& d, size_t t32, int sc) {
    return d.sbase + t32 * d.tstride + (sc & 1) * (32 * sizeof(uint4));
  }
  template <int KT, int NT> struct Frags {
    const char* ring;
    __device__ __forceinline__ Frags(const char* ring0, int lane) : ring(ring0 + wgtr_lane_off(lane)) {}
    __device__ __forceinline__ void read_a(int t, const half8& sc8, half8& h, half8& l) const {
      const char* p = ring + t * NP * 1024;
      h = tr_read8(p) * sc8;
      if constexpr (LO) l = tr_read8(p + 1024) * sc8;
    }
    __device__ __forceinline__ void read_b(int nt, half8& h, half8& l) const {
      const char* p = ring + (KT + nt) * NP * 1024;
      h = tr_read8(p);
      if constexpr (LO) l = tr_read8(p + 1024);
    }
  };
};

// RNERF_BWD_F16X3_LO8: f16 hi planes as above (block t = tile t), the lo planes as e4m3 bytes behind them.
// A lo tile of a 16-row step is 512 B in LDS, [row r][slot parity a][16 B = half 0 | half 1]; ONE DMA instruction builds TWO of them (lane
// L: tile L >> 5, row (L & 31) >> 1, parity L & 1 — 16 B = both halves of (slot, row), contiguous in the lo8 plane).  The 8-bit transpose
// read ds_read_b64_tr_b8 (within a 16-lane group destination lane i, byte j receives byte i & 7 of the 8 bytes addressed by source lane
// 2 j + (i >> 3): tools/ubench/tr8_cvt_probe.hip) hands lane (m = 16 a + i, kh) the 8 rows 8 kh .. 8 kh + 7 of feature position m in ONE
// read; four v_cvt_scalef32_pk_f16_fp8 turn them into the f16 lo fragment, and the three f16 MFMAs per product are those of the f16 lo
// planes — with the exact f16 hi parts in both cross terms.  Per step: (KT + NT) KiB of hi + (KT + NT) / 2 KiB of lo blocks.
__device__ __forceinline__ int2v tr_read8b(const char* p) {
  typedef __attribute__((address_space(3))) int2v lds_int2;
  return __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_int2*)p);
}
struct Lo8Planes {
  static constexpr bool LO = true;
  static constexpr int NPLANES = 2;
  static constexpr int NBUF = 4;      // ring depth (5 for the smaller steps measured slower: DESIGN.md section 3.3)
  static constexpr int nblk(int KT, int NT) { return KT + NT + (KT + 1) / 2 + (NT + 1) / 2; }
  static constexpr int lds_bytes() { return NBUF * wgtr_step_bytes(nblk(10, 8)); }
  template <int KT, int NT>
  static __device__ __forceinline__ WgTrDma dma(int b, int lane, const uint4* __restrict__ saved, const uint4* __restrict__ dy, long long R, const WgTrSegs& sg) {
    constexpr int NHI = KT + NT, NLX = (KT + 1) / 2;
    WgTrDma d;
    if (b < NHI) {                      // f16 hi block of tile b: as in F16Planes<1>
      const int r = lane >> 2, a = (lane >> 1) & 1, h = lane & 1;
      int s0, s1;
      const bool is_x = b < KT;
      if (is_x) x_slots(sg, b, s0, s1); else d_slots(sg, b - KT, s0, s1);
      d.sbase = (const char*)((is_x ? saved : dy) + sv_addr(__builtin_amdgcn_readfirstlane(s0), 0, 0, 0));
      d.voff = (unsigned)((sv_addr(a ? __builtin_amdgcn_readfirstlane(s1 - s0) : 0, 0, r, h)) * sizeof(uint4));
      d.tstride = (unsigned)((is_x ? SAVE_SLOTS : DY_SLOTS) * 64 * sizeof(uint4));
      d.hstride = (unsigned)(32 * sizeof(uint4));
      return d;
    }
    // e4m3 lo block: two tiles, lane = 32 (tile parity) + 2 r + a, 16 B = (slot a, row r, both halves)
    const int lb = b - NHI;
    const bool is_x = lb < NLX;
    const int t0 = 2 * (is_x ? lb : lb - NLX) + (lane >> 5);
    const int r = (lane & 31) >> 1, a = lane & 1;
    int s0, s1;
    if (is_x) x_slots(sg, t0 < KT ? t0 : KT - 1, s0, s1); else d_slots(sg, t0 < NT ? t0 : NT - 1, s0, s1);
    d.sbase = is_x ? (const char*)(saved + sv_lo0(R)) : (const char*)(dy + dy_plane_uint4(R, 1));
    d.voff = (unsigned)(((a ? s1 : s0) * 32 + r) * 16);
    d.tstride = (unsigned)((is_x ? SAVE_SLOTS : DY_SLOTS) * 32 * 16);
    d.hstride = 16u * 16u;
    return d;
  }
  static __device__ __forceinline__ const char* step_src(const WgTrDma& d, size_t t32, int sc) {
    return d.sbase + t32 * d.tstride + (sc & 1) * d.hstride;
  }
  template <int KT, int NT> struct Frags {
    static constexpr int LOX = (KT + NT) * 1024, LOD = LOX + (KT + 1) / 2 * 1024;      // the lo tiles of X / of dY
    const char *ring, *ring8;
    // lo tile: row (8 kh + (i >> 1)) * 32 + slot parity a * 16 + (i & 1) * 8, i = lane & 15
    __device__ __forceinline__ Frags(const char* ring0, int lane)
        : ring(ring0 + wgtr_lane_off(lane)), ring8(ring0 + (unsigned)((8 * (lane >> 5) + ((lane & 15) >> 1)) * 32 + ((lane >> 4) & 1) * 16 + (lane & 1) * 8)) {}
    __device__ __forceinline__ void read_a(int t, const half8& sc8, half8& h, half8& l) const {
      h = tr_read8(ring + t * 1024) * sc8;
      l = lo8_decode(tr_read8b(ring8 + LOX + t * 512), LO8_SCALE_X) * sc8;
    }
    __device__ __forceinline__ void read_b(int nt, half8& h, half8& l) const {
      h = tr_read8(ring + (KT + nt) * 1024);
      l = lo8_decode(tr_read8b(ring8 + LOD + nt * 512), LO8_SCALE_D);
    }
  };
};

template <class Planes, int KT, int NT>
__device__ __forceinline__ void wgrad_body_tr(const uint4* __restrict__ saved, const uint4* __restrict__ dy, long long R, float* __restrict__ pg,
                                               float* __restrict__ pbias, const WgTrSegs sg, int g, int G, char* smem) {
  using SH = WgTrShape<KT, NT>;
  constexpr int TK = SH::TK, TN = SH::TN;
  constexpr int NBLK = Planes::nblk(KT, NT), NDMA = (NBLK + 7) / 8, STEP_BYTES = wgtr_step_bytes(NBLK);
  constexpr int WGTR_NBUF = Planes::NBUF, AHEAD = WGTR_NBUF - 1;
  static_assert((WGTR_NBUF & (WGTR_NBUF - 1)) == 0, "ring slots are addressed with a mask");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wk = wave / SH::WN, wn = wave % SH::WN;
  const bool active = wave < SH::WK * SH::WN;
  const float* __restrict__ rs = (const float*)(dy + dy_plane_uint4(R, Planes::NPLANES));
  const float mref = rs[R];                                     // written by the dgrad's atomicMax
  const float inv_mref = mref > 0.f ? 1.0f / mref : 0.f;        // m_ref is a power of two: exact
  // DMA roles: block b = wave + 8 i (clamped: a surplus instruction re-fetches the last block, same bytes to the same place)
  WgTrDma blk[NDMA];
  unsigned lds_blk[NDMA];
#pragma unroll
  for (int i = 0; i < NDMA; ++i) {
    int b = wave + 8 * i;
    b = b < NBLK ? b : NBLK - 1;
    blk[i] = Planes::template dma<KT, NT>(b, lane, saved, dy, R, sg);
    lds_blk[i] = (unsigned)b * 1024u;
  }
  // the 16 row scales of a step ride the same ring (every VMEM operation of the loop is a DMA: one counter discipline): wave 0 fetches
  // them as one more DMA instruction, lanes 0..3 carry 4 floats each (the other lanes repeat them)
  const float* rs_src = rs + 4 * (lane & 3);
  const long long n_t32 = R / 32;
  const int my_tiles = g < n_t32 ? (int)((n_t32 - 1 - g) / G) + 1 : 0;
  const int n_steps = 2 * my_tiles;
  auto issue = [&](int s) {                                     // DMA of local step s into ring slot s & (WGTR_NBUF - 1) (steps past the end: the last one again)
    const int sc = s < n_steps ? s : n_steps - 1;
    const size_t t32 = (size_t)g + (size_t)(sc >> 1) * G;
    const unsigned ring = (unsigned)(s & (WGTR_NBUF - 1)) * STEP_BYTES;
#pragma unroll
    for (int i = 0; i < NDMA; ++i)
      glds16_nt_s(Planes::step_src(blk[i], t32, sc), blk[i].voff, __builtin_amdgcn_readfirstlane(ring + lds_blk[i]));
    if (wave == 0) glds16_nt((const char*)(rs_src + t32 * 32 + (sc & 1) * 16), __builtin_amdgcn_readfirstlane(ring + NBLK * 1024u));
  };
  const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  f32x16 acc[TK][TN], acce = zero;                         // acce: the extra tile (k-tile wk TK + wn) x (n-tile NT - 1)
  float accb = 0.f;                                        // bias row: this lane's share of sum_rows (m_row / m_ref) dY^[row][n] (VALU dot products)
#pragma unroll
  for (int i = 0; i < TK; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = zero;
  if (n_steps > 0) {
#pragma unroll
    for (int s = 0; s < AHEAD; ++s) issue(s);
    const int kh = lane >> 5;
    for (int s = 0; s < n_steps; ++s) {
      if (wave == 0) wait_vmcnt<(AHEAD - 1) * (NDMA + 1)>(); else
      wait_vmcnt<(AHEAD - 1) * NDMA>();                         // this wave's part of step s has landed (the later steps may be in flight)
      __syncthreads();                                          // ... everybody's has, and everybody is done with the ring slot of step s - 1
      // Every wave issues its DMA share (NDMA LDS-DMA instructions, ~100 issue cycles each) right behind the barrier.  The second wave of
      // every SIMD issuing it after its first chunk of MFMAs instead pays launched alone (f16x3 wgrad 2.008 / 2.010 -> 1.987 / 1.973 ms) but
      // not in the step, where the next batch's march shares those SIMDs (6.352 / 6.352 / 6.355 ms with it, 6.348 / 6.319 / 6.319 without;
      // DESIGN.md section 3.3, profiles/r06/ab_step_late_dma.txt)
      issue(s + AHEAD);
      if (active) {
        const char* ring0 = smem + (s & (WGTR_NBUF - 1)) * STEP_BYTES;
        const typename Planes::template Frags<KT, NT> frags(ring0, lane);
        const float4 s0 = *(const float4*)(ring0 + NBLK * 1024 + kh * 32), s1 = *(const float4*)(ring0 + NBLK * 1024 + kh * 32 + 16);
        const half8 sc8 = {(_Float16)(s0.x * inv_mref), (_Float16)(s0.y * inv_mref), (_Float16)(s0.z * inv_mref), (_Float16)(s0.w * inv_mref),
                           (_Float16)(s1.x * inv_mref), (_Float16)(s1.y * inv_mref), (_Float16)(s1.z * inv_mref), (_Float16)(s1.w * inv_mref)};
        // Operands are fetched and consumed in chunks so that the live set beside the TK x TN accumulators stays small enough for
        // WGRAD_VGPRS without spilling: the smaller operand side stays resident for the step, the other side streams through in
        // chunks (A fragments one k-tile at a time when TK > TN, else B fragments NCH n-tiles at a time).
        half8 beh, bel;                     // the B fragments of the extra tile's n-tile
        if constexpr (SH::EXTRA) frags.read_b(NT - 1, beh, bel);
        static_assert(SH::WK >= TN, "bias owners");
        auto read_a = [&](int i, half8& h, half8& l) { frags.read_a(wk * TK + i, sc8, h, l); };
        auto read_b = [&](int j, half8& h, half8& l) { frags.read_b(wn * TN + j, h, l); };
        // bias row: wave (wk, wn) owns it for n-tile wn TN + wk, wk < TN (the 9th n-tile of the Dense_9 + sigma job has no owner: the
        // sigma bias comes out of the rgb-head job, which reads the same head-gradient slot).  A B fragment holds, per lane, 8 rows of one
        // column and sc8 the scales of the same 8 rows: four v_dot2_f32_f16 per fragment instead of an MFMA with a one-row A operand and
        // a 16-register accumulator (the kernel has to stay within WGRAD_VGPRS).
        auto dot8 = [&](const half8& x, float c) -> float {
#pragma unroll
          for (int k = 0; k < 4; ++k) c = __builtin_amdgcn_fdot2(half2v{sc8[2 * k], sc8[2 * k + 1]}, half2v{x[2 * k], x[2 * k + 1]}, c, false);
          return c;
        };
        auto bias_row = [&](int j, const half8& h, const half8& l) {
          if (wk == j) {
            accb = dot8(h, accb);
            if constexpr (Planes::LO) accb = dot8(l, accb);
          }
        };
        half8 ae_h, ae_l;                   // the A fragments of the extra tile's k-tile (EXTRA: TK == 2, A side resident)
        if constexpr (TK > TN) {            // B resident, A streams
          half8 bh[TN], bl[TN];
#pragma unroll
          for (int j = 0; j < TN; ++j) read_b(j, bh[j], bl[j]);
          half8 an_h, an_l;
          read_a(0, an_h, an_l);
#pragma unroll
          for (int i = 0; i < TK; ++i) {
            const half8 ah = an_h, al = an_l;
            if (i + 1 < TK) read_a(i + 1, an_h, an_l);         // the next k-tile's fragments are on their way while this one's MFMAs issue
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = mfma_h8(ah, bh[j], acc[i][j]);
            if constexpr (Planes::LO) {
#pragma unroll
              for (int j = 0; j < TN; ++j) acc[i][j] = mfma_h8(ah, bl[j], acc[i][j]);
#pragma unroll
              for (int j = 0; j < TN; ++j) acc[i][j] = mfma_h8(al, bh[j], acc[i][j]);
            }
          }
#pragma unroll
          for (int j = 0; j < TN; ++j) bias_row(j, bh[j], bl[j]);
        } else {                            // A resident, B streams in chunks of NCH n-tiles
          constexpr int NCH = WGTR_NCH < TN ? WGTR_NCH : TN;
          static_assert(TN % NCH == 0, "n-tile chunks");
          half8 ah[TK], al[TK];
#pragma unroll
          for (int i = 0; i < TK; ++i) read_a(i, ah[i], al[i]);
#pragma unroll
          for (int c = 0; c < TN / NCH; ++c) {
            half8 bh[NCH], bl[NCH];
#pragma unroll
            for (int jj = 0; jj < NCH; ++jj) read_b(c * NCH + jj, bh[jj], bl[jj]);
#pragma unroll
            for (int i = 0; i < TK; ++i)
#pragma unroll
              for (int jj = 0; jj < NCH; ++jj) acc[i][c * NCH + jj] = mfma_h8(ah[i], bh[jj], acc[i][c * NCH + jj]);
            if constexpr (Planes::LO) {
#pragma unroll
              for (int i = 0; i < TK; ++i)
#pragma unroll
                for (int jj = 0; jj < NCH; ++jj) acc[i][c * NCH + jj] = mfma_h8(ah[i], bl[jj], acc[i][c * NCH + jj]);
#pragma unroll
              for (int i = 0; i < TK; ++i)
#pragma unroll
                for (int jj = 0; jj < NCH; ++jj) acc[i][c * NCH + jj] = mfma_h8(al[i], bh[jj], acc[i][c * NCH + jj]);
            }
#pragma unroll
            for (int jj = 0; jj < NCH; ++jj) bias_row(c * NCH + jj, bh[jj], bl[jj]);
          }
          if constexpr (SH::EXTRA) { ae_h = wn ? ah[1] : ah[0]; if constexpr (Planes::LO) ae_l = wn ? al[1] : al[0]; }
        }
        if constexpr (SH::EXTRA) {          // wn picks which of the wave's two k-tiles (a select on registers, no branch)
          static_assert(!SH::EXTRA || TK <= TN, "the extra tile reads the resident A fragments");
          acce = mfma_h8(ae_h, beh, acce);
          if constexpr (Planes::LO) {
            acce = mfma_h8(ae_h, bel, acce);
            acce = mfma_h8(ae_l, beh, acce);
          }
        }
      }
    }
    wait_vmcnt<0>();                                            // the surplus prefetches must not outlive the workgroup's LDS
  }
  constexpr size_t ldn = (size_t)NT * 32;
  const int m = lane & 31, h = lane >> 5;
  if (active) {
#pragma unroll
    for (int i = 0; i < TK; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
          pg[(size_t)((wk * TK + i) * 32 + row) * ldn + (wn * TN + j) * 32 + m] = acc[i][j][r];
        }
    if constexpr (SH::EXTRA) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        pg[(size_t)((wk * TK + wn) * 32 + row) * ldn + (NT - 1) * 32 + m] = acce[r];
      }
    }
    const float bsum = accb + __shfl_xor(accb, 32);          // the two 8-row halves of a k-step live in lanes m and m + 32
    if (wk < TN && h == 0) pbias[(wn * TN + wk) * 32 + m] = bsum;
  }
}

// At most 224 VGPRs per wave: two of these waves per SIMD then leave 64 registers — one wave of the march kernel — on every SIMD, so
// the next batch's march (a latency-bound chain that needs a wave slot on every CU, no LDS) can be co-resident with this HBM-paced kernel
// instead of waiting for whole CUs to drain.
constexpr int WGRAD_VGPRS = 112;      // the attribute counts half of the unified VGPR + AGPR file on gfx90a+: 112 -> 224 registers
template <class Planes>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_num_vgpr(WGRAD_VGPRS)))
nerfmlp_wgrad_tr_kernel(const uint4* __restrict__ saved, const uint4* __restrict__ dy, long long R, float* __restrict__ workspace, const WgradTable tab,
                        long long* __restrict__ trace) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if (trace && threadIdx.x == 0) trace[2 * blockIdx.x] = (long long)__builtin_amdgcn_s_memrealtime();
  int j = 0;
  while ((int)blockIdx.x >= tab.wg0[j + 1]) ++j;
  const WgradJob job = tab.job[j];
  const int g = blockIdx.x - tab.wg0[j], G = tab.wg0[j + 1] - tab.wg0[j];
  const int KT = job.KT, NT = job.NT;
  float* pg = workspace + tab.poff[j] + (size_t)g * (size_t)KT * 32 * NT * 32;
  float* pb = workspace + tab.pboff[j] + (size_t)g * NT * 32;
  const WgTrSegs sg = {tab.qx[j], job.KTa, tab.qx2[j], tab.qd[j], job.NTa, tab.KSd[j], tab.qd2[j], tab.KSd2[j]};
#define RNERF_WGRAD_CASE(KT_, NT_)                                                                                                  \
  if (KT == (KT_) && NT == (NT_)) {                                                                                                 \
    wgrad_body_tr<Planes, KT_, NT_>(saved, dy, R, pg, pb, sg, g, G, smem);                                                          \
    if (trace && threadIdx.x == 0) trace[2 * blockIdx.x + 1] = (long long)__builtin_amdgcn_s_memrealtime();                         \
    return;                                                                                                                         \
  }
  RNERF_WGRAD_CASE(8, 8) RNERF_WGRAD_CASE(2, 8) RNERF_WGRAD_CASE(10, 8) RNERF_WGRAD_CASE(8, 9) RNERF_WGRAD_CASE(9, 4) RNERF_WGRAD_CASE(4, 1)
#undef RNERF_WGRAD_CASE
  __builtin_trap();
}

template <bool X_F16>
__global__ void __launch_bounds__(512)
nerfmlp_wgrad_kernel(const uint4* __restrict__ saved, const uint4* __restrict__ dy, long long R, long long total_rows, int n_chunks,
                      float* __restrict__ workspace, const WgradTable tab) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int j = 0;
  while ((int)blockIdx.x >= tab.wg0[j + 1]) ++j;
  const int qx = tab.qx[j], KSx = tab.KSx[j], qd = tab.qd[j], KSd = tab.KSd[j];
  const int g = blockIdx.x - tab.wg0[j], G = tab.wg0[j + 1] - tab.wg0[j];
  const int KT = KSx >> 1, NT = (KSd + 1) >> 1;
  float* pg = workspace + tab.poff[j] + (size_t)g * (size_t)KT * 32 * NT * 32;
  float* pb = workspace + tab.pboff[j] + (size_t)g * NT * 32;
#define RNERF_WGRAD_CASE(KT_, KSD_)                                                                                                 \
  if (KSx == 2 * (KT_) && KSd == (KSD_)) { wgrad_body<X_F16, KT_, KSD_>(saved, dy, R, total_rows, n_chunks, pg, pb, qx, qd, g, G, smem); return; }
  RNERF_WGRAD_CASE(8, 16) RNERF_WGRAD_CASE(2, 16) RNERF_WGRAD_CASE(8, 1) RNERF_WGRAD_CASE(8, 8) RNERF_WGRAD_CASE(1, 8) RNERF_WGRAD_CASE(4, 1)
#undef RNERF_WGRAD_CASE
  __builtin_trap();
}

__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* __restrict__ workspace, const WgradTable tab, float* __restrict__ grads,
                                                           const float* __restrict__ out_scale) {
  const float osc = out_scale ? *out_scale : 1.0f;      // m_ref of the row-normalised modes
  const int jb = blockIdx.y;
  const WgradJob job = tab.job[jb];
  const int n_wg = tab.wg0[jb + 1] - tab.wg0[jb];
  const float* __restrict__ partial = workspace + tab.poff[jb];
  const float* __restrict__ partial_bias = workspace + tab.pboff[jb];
  const int ldn = job.NT * 32, rows = job.KT * 32;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  // column J of the partial -> (Dense index, output feature) through the dY segment it lies in
  auto out_feature = [&](int J, int& dense) -> int {
    int nt = J >> 5;
    const int c = J & 31, a = c >> 4, hh = (c >> 3) & 1, j = c & 7;
    const bool segb = nt >= job.NTa;
    const int dkind = segb ? job.dkind2 : job.dkind;
    dense = segb ? job.dense2 : job.dense;
    if (segb) nt -= job.NTa;
    if (dkind == 0) { const int n = prev_feature(2 * nt + a, hh, j); return n < nerf_dense(dense).out ? n : -1; }
    if (a != 0 || hh != 0 || nt != 0) return -1;
    if (dkind == 1) return j == 0 ? 0 : -1;
    return (j >= 1 && j <= 3) ? j - 1 : -1;
  };
  auto sum_over = [&](const float* __restrict__ p, size_t stride) -> float {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int g = 0;
    for (; g + 4 <= n_wg; g += 4) { s0 += p[(size_t)g * stride]; s1 += p[(size_t)(g + 1) * stride]; s2 += p[(size_t)(g + 2) * stride]; s3 += p[(size_t)(g + 3) * stride]; }
    for (; g < n_wg; ++g) s0 += p[(size_t)g * stride];
    return (s0 + s1) + (s2 + s3);
  };
  if (e < rows * ldn) {
    const int I = e / ldn, J = e % ldn;
    int kt = I >> 5;
    const int c = I & 31, a = c >> 4, hh = (c >> 3) & 1, j = c & 7;
    const bool segb = kt >= job.KTa;
    const int xkind = segb ? job.xkind2 : job.xkind, row_off = segb ? job.row_off2 : job.row_off;
    if (segb) kt -= job.KTa;
    const int s = 2 * kt + a;
    int fin = xkind == 1 ? prev_feature(s, hh, j) : (xkind == 0 ? pe_feature(8 * s + j, hh) : view_feature(8 * s + j, hh));
    int dense;
    const int fout = out_feature(J, dense);
    if (fin >= 0 && fout >= 0) {
      fin += row_off;
      if (fin < nerf_dense(dense).in) grads[nerf_koff(dense) + fin * nerf_dense(dense).out + fout] = sum_over(partial + e, (size_t)rows * ldn) * osc;
    }
  }
  if (job.write_bias && e < ldn) {
    int dense;
    const int fout = out_feature(e, dense);
    if (fout >= 0 && (e >> 5) < job.NTa) grads[nerf_boff(dense) + fout] = sum_over(partial_bias + e, (size_t)ldn) * osc;
    if (job.bias_sigma && e == 0) grads[nerf_boff(8)] = sum_over(partial_bias, (size_t)ldn) * osc;      // column 0 of the head slot = d raw_sigma
  }
}

// ---- d loss / d (position, direction) of every row of a NerfMLP level: through pos_enc (rnerf/model_utils.py:187-214) into Dense_0, the
// skip concat of Dense_5 (:68-69) and the view layer Dense_10 (:82-87).  One wave = 32 rows; exact fp32 MFMA on the (normalised, f16)
// gradients the dgrad chain left in `dy`, rescaled by the row scale.
template <int NP>
__global__ void __launch_bounds__(64) nerfmlp_input_grad_kernel(const float* __restrict__ params, const uint4* __restrict__ dy, long long R,
                                                                const float4* __restrict__ rows_pd, const float4* __restrict__ rows_dr,
                                                                const int* __restrict__ node_of_sample, int B, long long total_rows,
                                                                float4* __restrict__ d_pos, float4* __restrict__ d_dir) {
  const int lane = threadIdx.x & 63, m = lane & 31, h = lane >> 5;
  long long row = (long long)blockIdx.x * 32 + m;
  const bool ok = row < total_rows;
  if (!ok) row = total_rows - 1;
  const f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  f32x16 dpe[2] = {zero, zero}, dve = zero;
  // B operand of MFMA j of slot q: the gradient of feature prev_feature(s, h, j) of this lane's row (hi [+ lo] f16 parts)
  auto slot_vals = [&](int q, float (&vals)[8]) {
    const uint4 hi = dy[dy_addr(q, row >> 5, (int)(row & 31), h)];
    const uint32_t hw[4] = {hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int p = 0; p < 4; ++p) unpack2<true>(hw[p], vals[2 * p], vals[2 * p + 1]);
    if constexpr (NP == 2) {
      const uint4 lo = dy[dy_plane_uint4(R, 1) + dy_addr(q, row >> 5, (int)(row & 31), h)];
      const uint32_t lw[4] = {lo.x, lo.y, lo.z, lo.w};
#pragma unroll
      for (int p = 0; p < 4; ++p) { float a, b; unpack2<true>(lw[p], a, b); vals[2 * p] += a; vals[2 * p + 1] += b; }
    }
    if constexpr (NP == 3) {      // RNERF_BWD_F16X3_LO8: the lo parts as e4m3 bytes (lo8_pack), 8 B per (row, half)
      const uint2 lo = ((const uint2*)(dy + dy_plane_uint4(R, 1)))[dy_addr(q, row >> 5, (int)(row & 31), h)];
      const half8 lv = lo8_decode(int2v{(int)lo.x, (int)lo.y}, LO8_SCALE_D);
#pragma unroll
      for (int j = 0; j < 8; ++j) vals[j] += (float)lv[j];
    }
  };
  // The kernel rows a lane needs for one slot are 8 consecutive floats (two 16-byte loads per n-tile), and neither they nor the dY
  // operands depend on the accumulators: slot s + 1 is fetched while the 8 x ntile MFMAs of slot s run (one dword load + vmcnt(0) per MFMA
  // before: 0.76 ms per 524 k rows, three times the matrix time).
  auto gemm_T = [&](const float* __restrict__ kern, int out_dim, int row0, int fin, int slot0, int nslots, f32x16* acc, int ntile) {
    const float* __restrict__ kr[2];
    bool live[2];
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      const int f = 32 * t2 + m;
      live[t2] = f < fin;
      kr[t2] = kern + (size_t)(row0 + (f < fin ? f : fin - 1)) * out_dim + 4 * h;
    }
    float4 wc[2][2], wn[2][2];
    float vc[8], vn[8];
    auto fetch = [&](int s, float4 (&w)[2][2], float (&vals)[8]) {
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
        if (t2 < ntile) { w[t2][0] = *(const float4*)(kr[t2] + 16 * s); w[t2][1] = *(const float4*)(kr[t2] + 16 * s + 8); }
      slot_vals(slot0 + s, vals);
    };
    fetch(0, wc, vc);
#pragma unroll 1
    for (int s = 0; s < nslots; ++s) {
      if (s + 1 < nslots) fetch(s + 1, wn, vn);
      RNERF_PIN();
#pragma unroll
      for (int j = 0; j < 8; ++j) {                                  // feature prev_feature(s, h, j) = 16 s + 8 (j >> 2) + 4 h + (j & 3)
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) {
          if (t2 < ntile) {
            const float4 q = wc[t2][j >> 2];
            const float w = (j & 3) == 0 ? q.x : ((j & 3) == 1 ? q.y : ((j & 3) == 2 ? q.z : q.w));
            acc[t2] = __builtin_amdgcn_mfma_f32_32x32x2f32(live[t2] ? w : 0.f, vc[j], acc[t2], 0, 0, 0);
          }
        }
      }
      RNERF_PIN();
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) { wc[t2][0] = wn[t2][0]; wc[t2][1] = wn[t2][1]; }
#pragma unroll
      for (int j = 0; j < 8; ++j) vc[j] = vn[j];
    }
  };
  gemm_T(params + nerf_koff(0), 256, 0, 63, 0, 16, dpe, 2);                 // Dense_0: pos_enc -> 256, dY_0 = slots 0..15
  gemm_T(params + nerf_koff(5), 256, 256, 63, 16 * 5, 16, dpe, 2);          // Dense_5 rows 256..318 (skip concat), dY_5 = slots 80..95
  gemm_T(params + nerf_koff(10), 128, 256, 27, DY_L9, 8, &dve, 1);          // Dense_10 rows 256..282 (view encoding), dY_9 = slots 144..151
  size_t rec = (size_t)row;
  if (node_of_sample) { const long long sidx = row / B; rec = (size_t)node_of_sample[sidx] * B + (size_t)(row - sidx * B); }
  const float4 pd = rows_pd[rec], dr = rows_dr[rec];
  const float pc[3] = {pd.x, pd.y, pd.z}, dcv[3] = {dr.x, dr.y, dr.z};
  const float HALF_PI = 1.5707963705062866f;
  // (pe_cos: the forward's Cephes-grade reduction + polynomial, ~25 VALU ops; ocml's cosf is ~100 and there are 44 per lane)
  float gp3[3] = {0.f, 0.f, 0.f}, gd3[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int f = 32 * t2 + (r & 3) + 8 * (r >> 2) + 4 * h;          // pos_enc feature: [x(3) | sin(2^d x)(30) | sin(2^d x + pi/2)(30)]
      if (f < 3) gp3[f] += dpe[t2][r];
      else if (f < 63) {
        const int q = (f - 3) % 30, is_cos = (f - 3) / 30, d = q / 3, c = q % 3;
        const float xb = fmul(pc[c], (float)(1 << d));
        gp3[c] = fmaf(dpe[t2][r], (float)(1 << d) * pe_cos(is_cos ? fadd(xb, HALF_PI) : xb), gp3[c]);
      }
    }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int f = (r & 3) + 8 * (r >> 2) + 4 * h;                      // view enc feature: [d(3) | sin (12) | cos (12)]
    if (f < 3) gd3[f] += dve[r];
    else if (f < 27) {
      const int q = (f - 3) % 12, is_cos = (f - 3) / 12, d = q / 3, c = q % 3;
      const float xb = fmul(dcv[c], (float)(1 << d));
      gd3[c] = fmaf(dve[r], (float)(1 << d) * pe_cos(is_cos ? fadd(xb, HALF_PI) : xb), gd3[c]);
    }
  }
  const float* __restrict__ rs = (const float*)(dy + dy_plane_uint4(R, NP == 3 ? 2 : NP));
  const float sc = rs[row];                                            // the gradients in dy are d / m_row
#pragma unroll
  for (int c = 0; c < 3; ++c) { gp3[c] = (gp3[c] + __shfl_xor(gp3[c], 32)) * sc; gd3[c] = (gd3[c] + __shfl_xor(gd3[c], 32)) * sc; }
  if (ok && h == 0) { d_pos[row] = make_float4(gp3[0], gp3[1], gp3[2], 0.f); d_dir[row] = make_float4(gd3[0], gd3[1], gd3[2], 0.f); }
}

}  // namespace rnerf

namespace rnerf {
// csrc/mlp_f32.hip: the exact-fp32 arbiter (RNERF_PREC_F32)
int launch_fwd_f32(const void* packed, const float* rows_pd, const float* rows_dr, const int32_t* node_of_sample, int32_t B, long long total_rows,
                   float* out_raw, hipStream_t st);
}

using namespace rnerf;

// f16f8 packs TWO streams: its own, and behind it (256-byte aligned) the f16x3 stream a launch falls back to when a weight is out of its range
constexpr size_t kF8Fallback = (Prec<RNERF_PREC_F16F8>::PACKED_BYTES + 255) & ~(size_t)255;

// Every f16-based EVALUATION stream is followed (256-byte aligned) by a bf16x3 stream of the same weights: the range-safe second pass of
// rnerf_nerfmlp_forward (nerfmlp_fwd_kernel's REDO mode) recomputes, in fp32's exponent range, the rows the f16 pass returned as NaN.
constexpr size_t kX3Bytes = (Prec<RNERF_PREC_F16X3>::PACKED_BYTES + 255) & ~(size_t)255;
constexpr size_t kSafeBytes = Prec<RNERF_PREC_BF16X3>::PACKED_BYTES;
constexpr size_t kF16Bytes = (Prec<RNERF_PREC_F16>::PACKED_BYTES + 255) & ~(size_t)255;
static size_t safe_stream_offset(int precision) {      // offset of that bf16x3 stream in a packed buffer of `precision` (0: it has none)
  switch (precision) {
    case RNERF_PREC_F16X3:
    case RNERF_PREC_F16X2: return kX3Bytes;
    case RNERF_PREC_F16F8: return kF8Fallback + kX3Bytes;
    case RNERF_PREC_F16: return kF16Bytes;
    default: return 0;
  }
}

#define RNERF_TRY_(expr) do { int rc_ = (expr); if (rc_ != RNERF_OK) return rc_; } while (0)

static bool prec_ok(int p) {
  return p == RNERF_PREC_F32 || p == RNERF_PREC_F16X3 || p == RNERF_PREC_BF16X3 || p == RNERF_PREC_F16 || p == RNERF_PREC_BF16 || p == RNERF_PREC_F16X2 || p == RNERF_PREC_F16F8;
}

extern "C" size_t rnerf_nerfmlp_packed_bytes(int precision) {
  switch (precision) {
    case RNERF_PREC_F32: return (size_t)RNERF_NERFMLP_PARAMS * sizeof(float);  // the flat fp32 buffer itself
    case RNERF_PREC_F16X3:
    case RNERF_PREC_F16X2: return kX3Bytes + kSafeBytes;                      // f16x2 reads the f16x3 stream; + the range-safe bf16x3 stream
    case RNERF_PREC_F16F8: return kF8Fallback + kX3Bytes + kSafeBytes;        // its own stream, the f16x3 stream it falls back to, the bf16x3 stream
    case RNERF_PREC_BF16X3: return Prec<RNERF_PREC_BF16X3>::PACKED_BYTES;
    case RNERF_PREC_F16: return kF16Bytes + kSafeBytes;                       // the single-pass stream + the range-safe bf16x3 stream
    case RNERF_PREC_BF16: return Prec<RNERF_PREC_BF16>::PACKED_BYTES;
    default: set_error("rnerf_nerfmlp_packed_bytes: unsupported precision %d", precision); return 0;
  }
}

namespace rnerf {
void* nerfmlp_dgrad_scale_ref(int backward, void* dy, int64_t rows);      // (defined with the dgrad launcher below)
// the range flag(s) of a packed stream: 4 floats behind the aux block of every f16 stream (f16f8: its own and its f16x3 fallback's)
static int pack_flag_regions(int precision, void* packed, void** out) {
  auto at = [&](size_t off) { return (void*)((char*)packed + off + AUX_FLAG * sizeof(float)); };
  switch (precision) {
    case RNERF_PREC_F16X3:
    case RNERF_PREC_F16X2: out[0] = at(Prec<RNERF_PREC_F16X3>::STREAM_BYTES); return 1;
    case RNERF_PREC_F16F8: out[0] = at(Prec<RNERF_PREC_F16F8>::STREAM_BYTES); out[1] = at(kF8Fallback + Prec<RNERF_PREC_F16X3>::STREAM_BYTES); return 2;
    case RNERF_PREC_F16: out[0] = at(Prec<RNERF_PREC_F16>::STREAM_BYTES); return 1;
    default: return 0;
  }
}
struct FlagRegions { float4* p[12]; };
__global__ void __launch_bounds__(64) zero_flags_kernel(FlagRegions r, int n) {
  if ((int)threadIdx.x < n) *r.p[threadIdx.x] = make_float4(0.f, 0.f, 0.f, 0.f);
}
// Zeroes, in ONE launch, every 16-byte accumulator / flag word a training step needs cleared before its kernels run: the range flags of
// the operand streams it packs (`packed`, `count` <= 2) and the row-scale reference of each dgrad's dY buffer (`dy` / `dy_rows`, see
// launch_dgrad).  As hipMemsetAsync calls inside the producers each was a fill kernel of its own, ~6 us apiece with its launch gap, on
// the main stream's dependent chain (round 4; the env-map sum and sum theta^2 became fixed-order reductions that need no clearing).
int nerfmlp_step_zero(int precision, void* const* packed, int count, int backward, void* const* dy, const int64_t* dy_rows, int dy_count, hipStream_t st) {
  FlagRegions r;
  int n = 0;
  for (int i = 0; i < count && i < 2; ++i) { void* o[2]; const int k = pack_flag_regions(precision, packed[i], o); for (int q = 0; q < k; ++q) r.p[n++] = (float4*)o[q]; }
  for (int i = 0; i < dy_count && i < 4; ++i) { void* f = nerfmlp_dgrad_scale_ref(backward, dy[i], dy_rows[i]); if (f) r.p[n++] = (float4*)f; }
  if (n == 0) return RNERF_OK;
  hipLaunchKernelGGL(zero_flags_kernel, dim3(1), dim3(64), 0, st, r, n);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

// zero_flags = false: the caller has zeroed the stream's range flags on `stream` already (nerfmlp_pack_zero_flags)
// with_safe = false: leave the range-safe bf16x3 stream of an f16-based buffer unwritten (the training step's own streams: the training
// forward has no second pass — a row out of range reaches the non-finite-gradient count instead)
int nerfmlp_pack_impl(const float* params, int precision, void* packed, bool zero_flags, hipStream_t st, bool with_safe) {
  const int threads = kTotalBlocks * 64, block = 256, grid = (threads + block - 1) / block;
  if (zero_flags) {
    void* o[2];
    const int k = pack_flag_regions(precision, packed, o);
    for (int q = 0; q < k; ++q) RNERF_CHECK_HIP(hipMemsetAsync(o[q], 0, 4 * sizeof(float), st));
  }
  switch (precision) {
    case RNERF_PREC_F32:
      RNERF_CHECK_HIP(hipMemcpyAsync(packed, params, (size_t)RNERF_NERFMLP_PARAMS * sizeof(float), hipMemcpyDeviceToDevice, st));
      return RNERF_OK;
    case RNERF_PREC_F16X3:
    case RNERF_PREC_F16X2: hipLaunchKernelGGL(nerfmlp_pack_kernel<RNERF_PREC_F16X3>, dim3(grid), dim3(block), 0, st, params, (char*)packed); break;
    case RNERF_PREC_F16F8:
      hipLaunchKernelGGL(nerfmlp_pack_kernel<RNERF_PREC_F16F8>, dim3(grid), dim3(block), 0, st, params, (char*)packed);
      hipLaunchKernelGGL(nerfmlp_pack_kernel<RNERF_PREC_F16X3>, dim3(grid), dim3(block), 0, st, params, (char*)packed + kF8Fallback);
      break;
    case RNERF_PREC_F16: hipLaunchKernelGGL(nerfmlp_pack_kernel<RNERF_PREC_F16>, dim3(grid), dim3(block), 0, st, params, (char*)packed); break;
    case RNERF_PREC_BF16X3: hipLaunchKernelGGL(nerfmlp_pack_kernel<RNERF_PREC_BF16X3>, dim3(grid), dim3(block), 0, st, params, (char*)packed); break;
    default: hipLaunchKernelGGL(nerfmlp_pack_kernel<RNERF_PREC_BF16>, dim3(grid), dim3(block), 0, st, params, (char*)packed); break;
  }
  if (with_safe && safe_stream_offset(precision) != 0)
    hipLaunchKernelGGL(nerfmlp_pack_kernel<RNERF_PREC_BF16X3>, dim3(grid), dim3(block), 0, st, params, (char*)packed + safe_stream_offset(precision));
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}
}  // namespace rnerf

extern "C" int rnerf_nerfmlp_pack(const float* params, int precision, void* packed, void* stream) {
  RNERF_CHECK_ARG(params && packed, "rnerf_nerfmlp_pack: null pointer");
  RNERF_CHECK_ARG(prec_ok(precision), "rnerf_nerfmlp_pack: unsupported precision %d", precision);
  RNERF_CHECK_ARG(((uintptr_t)packed & 15) == 0, "rnerf_nerfmlp_pack: packed must be 16-byte aligned");
  return nerfmlp_pack_impl(params, precision, packed, true, (hipStream_t)stream, true);
}

// saved operands + masks of `padded` rows; behind them SAVE_QUEUE_BYTES for the dynamic tile queue of a capped training forward
constexpr size_t SAVE_QUEUE_BYTES = 8192;       // counter + one slot per workgroup (<= 2047 CUs)
static size_t save_payload_bytes(long long padded, bool with_lo) {
  return (size_t)(SAVE_TOTAL + (with_lo ? SAVE_SLOTS : 0)) * (size_t)padded * 2 * sizeof(uint4);
}

// MODE: 0 = the pass, 512 = the range-safe second pass (REDO in nerfmlp_fwd_kernel); TRAIN: see nerfmlp_fwd_kernel
template <int PREC, int MODE = 0, int TRAIN = 0>
static int launch_fwd_mode(const void* packed, const float* rows_pd, const float* rows_dr, const int32_t* node_of_sample, int32_t B,
                           long long total_rows, float* out_raw, hipStream_t st, void* save = nullptr, int max_wg = 0, const float* gate = nullptr,
                           int gate_skip_if = 0) {
  using PP = Prec<PREC>;
  const int n_tiles = (int)((total_rows + 255) / 256);
  int dev = 0, cus = 0;
  RNERF_CHECK_HIP(hipGetDevice(&dev));
  RNERF_CHECK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const int lim = (max_wg > 0 && max_wg < cus) ? max_wg : cus;
  // Few rows: 128-row tiles (one m-tile per wave) when all of them fit ONE round of workgroups — a tile's time is the serial work of its
  // waves, so a launch that cannot fill the chip with 256-row tiles (a 512-ray shard's coarse level: 128 tiles on 256 CUs; both levels of a
  // 128-ray one) finishes sooner on twice as many CUs with half the work each.  (Beyond one round the 256-row tiles' better reuse of the
  // weight stream wins.)  RNERF_FWD_HALF_TILES=0 switches it off (A/B).
  if constexpr (MODE == 0 && (PREC == RNERF_PREC_F16X3 || PREC == RNERF_PREC_F16F8)) {
    static const bool half_ok = [] { const char* e = RNERF_ENV("RNERF_FWD_HALF_TILES"); return !(e && e[0] == '0'); }();
    if (half_ok && 2 * n_tiles <= lim) {
      const size_t lds1 = 2 * (size_t)PP::SLAB;
      static DeviceOnce attr1_set;
      if (attr1_set.need()) {
        RNERF_CHECK_HIP(hipFuncSetAttribute((const void*)nerfmlp_fwd_kernel<PREC, 0, TRAIN, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1));
        attr1_set.set();
      }
      hipLaunchKernelGGL((nerfmlp_fwd_kernel<PREC, 0, TRAIN, true>), dim3(2 * n_tiles), dim3(256), lds1, st, (const char*)packed, (const float4*)rows_pd,
                         (const float4*)rows_dr, node_of_sample, B, total_rows, 2 * n_tiles, (float4*)out_raw, (uint4*)save, (long long)n_tiles * 256,
                         (int*)nullptr, gate, gate_skip_if);
      RNERF_CHECK_LAUNCH();
      return RNERF_OK;
    }
  }
  const int grid = n_tiles < lim ? n_tiles : lim;
  const size_t lds = 2 * (size_t)PP::SLAB + 4 * 32768;
  static DeviceOnce attr_set;
  if (attr_set.need()) {
    RNERF_CHECK_HIP(hipFuncSetAttribute((const void*)nerfmlp_fwd_kernel<PREC, MODE, TRAIN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set.set();
  }
  int* tileq = nullptr;
  if (TRAIN != 0 && grid < cus && grid < n_tiles) {      // capped training forward: dynamic tile queue in the tail of the save buffer
    tileq = (int*)((char*)save + save_payload_bytes((long long)n_tiles * 256, TRAIN >= 2));
    RNERF_CHECK_HIP(hipMemsetAsync(tileq, 0, sizeof(int), st));
  }
  hipLaunchKernelGGL((nerfmlp_fwd_kernel<PREC, MODE, TRAIN>), dim3(grid), dim3(256), lds, st, (const char*)packed, (const float4*)rows_pd,
                     (const float4*)rows_dr, node_of_sample, B, total_rows, n_tiles, (float4*)out_raw, (uint4*)save,
                     (long long)n_tiles * 256, tileq, gate, gate_skip_if);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

template <int PREC>
static int launch_fwd(const void* packed, const float* rows_pd, const float* rows_dr, const int32_t* node_of_sample, int32_t B,
                      long long total_rows, float* out_raw, hipStream_t st, int max_wg, const float* gate = nullptr, int gate_skip_if = 0) {
  return launch_fwd_mode<PREC>(packed, rows_pd, rows_dr, node_of_sample, B, total_rows, out_raw, st, nullptr, max_wg, gate, gate_skip_if);
}

extern "C" int rnerf_nerfmlp_forward(const void* packed, int precision, const float* rows_pd, const float* rows_dr,
                                     const int32_t* node_of_sample, int32_t S, int32_t B, float* out_raw, int32_t max_workgroups,
                                     void* stream) {
  RNERF_CHECK_ARG(packed && rows_pd && rows_dr && out_raw, "rnerf_nerfmlp_forward: null pointer");
  RNERF_CHECK_ARG(max_workgroups >= 0, "rnerf_nerfmlp_forward: max_workgroups must be >= 0");
  RNERF_CHECK_ARG(prec_ok(precision), "rnerf_nerfmlp_forward: unsupported precision %d", precision);
  RNERF_CHECK_ARG(S >= 1 && B >= 1, "rnerf_nerfmlp_forward: need S >= 1 and B >= 1");
  RNERF_CHECK_ARG((((uintptr_t)packed | (uintptr_t)rows_pd | (uintptr_t)rows_dr | (uintptr_t)out_raw) & 15) == 0,
                  "rnerf_nerfmlp_forward: buffers must be 16-byte aligned");
  const long long total = (long long)S * B;
  hipStream_t st = (hipStream_t)stream;
  switch (precision) {
    case RNERF_PREC_F32: return launch_fwd_f32(packed, rows_pd, rows_dr, node_of_sample, B, total, out_raw, st);
    // every f16-based launch is followed by the range-safe second pass: bf16x3 (fp32's exponent range) on the rows the first pass returned
    // as NaN — an activation above f16's 65504, a weight >= 256 —, nothing else touched; without such a row it reads out_raw once and ends
    case RNERF_PREC_F16X3:
      RNERF_TRY_(launch_fwd<RNERF_PREC_F16X3>(packed, rows_pd, rows_dr, node_of_sample, B, total, out_raw, st, max_workgroups));
      return launch_fwd_mode<RNERF_PREC_BF16X3, 512>((const char*)packed + safe_stream_offset(precision), rows_pd, rows_dr, node_of_sample, B, total, out_raw, st, nullptr, max_workgroups);
    case RNERF_PREC_F16X2:
      RNERF_TRY_(launch_fwd<RNERF_PREC_F16X2>(packed, rows_pd, rows_dr, node_of_sample, B, total, out_raw, st, max_workgroups));
      return launch_fwd_mode<RNERF_PREC_BF16X3, 512>((const char*)packed + safe_stream_offset(precision), rows_pd, rows_dr, node_of_sample, B, total, out_raw, st, nullptr, max_workgroups);
    case RNERF_PREC_F16F8: {
      // the f16f8 launch steps aside when its pack kernel flagged a weight outside the range of the 2^14-scaled stream (|W| >= 3.99); the f16x3
      // launch behind it (its stream sits in the same packed buffer) runs only then: a fallback per launch, decided on the device
      const float* flag = (const float*)((const char*)packed + Prec<RNERF_PREC_F16F8>::STREAM_BYTES) + AUX_FLAG;
      RNERF_TRY_(launch_fwd<RNERF_PREC_F16F8>(packed, rows_pd, rows_dr, node_of_sample, B, total, out_raw, st, max_workgroups, flag, 1));
      RNERF_TRY_(launch_fwd<RNERF_PREC_F16X3>((const char*)packed + kF8Fallback, rows_pd, rows_dr, node_of_sample, B, total, out_raw, st, max_workgroups, flag, 0));
      return launch_fwd_mode<RNERF_PREC_BF16X3, 512>((const char*)packed + safe_stream_offset(precision), rows_pd, rows_dr, node_of_sample, B, total, out_raw, st, nullptr, max_workgroups);
    }
    case RNERF_PREC_BF16X3: return launch_fwd<RNERF_PREC_BF16X3>(packed, rows_pd, rows_dr, node_of_sample, B, total, out_raw, st, max_workgroups);
    case RNERF_PREC_F16:
      RNERF_TRY_(launch_fwd<RNERF_PREC_F16>(packed, rows_pd, rows_dr, node_of_sample, B, total, out_raw, st, max_workgroups));
      return launch_fwd_mode<RNERF_PREC_BF16X3, 512>((const char*)packed + safe_stream_offset(precision), rows_pd, rows_dr, node_of_sample, B, total, out_raw, st, nullptr, max_workgroups);
    default: return launch_fwd<RNERF_PREC_BF16>(packed, rows_pd, rows_dr, node_of_sample, B, total, out_raw, st, max_workgroups);
  }
}

static bool bwd_ok(int b) { return b == RNERF_BWD_BF16 || b == RNERF_BWD_F16 || b == RNERF_BWD_F16X2 || b == RNERF_BWD_F16X3_LO8; }
static bool bwd_two_planes(int b) { return b == RNERF_BWD_F16X2 || b == RNERF_BWD_F16X3_LO8; }      // (LO8: the lo planes use half of their region)
// (forward precision, backward mode) pairs the training kernels are built for
static bool train_combo_ok(int precision, int backward) {
  return precision == RNERF_PREC_F16X3 || (precision == RNERF_PREC_F16 && !bwd_two_planes(backward)) ||
         (precision == RNERF_PREC_BF16X3 && backward == RNERF_BWD_BF16);
}
static size_t train_stream_bytes(int precision) {      // the aux floats (biases, heads) sit behind the forward's operand stream
  return precision == RNERF_PREC_F16 ? Prec<RNERF_PREC_F16>::STREAM_BYTES : (precision == RNERF_PREC_BF16X3 ? Prec<RNERF_PREC_BF16X3>::STREAM_BYTES : Prec<RNERF_PREC_F16X3>::STREAM_BYTES);
}

extern "C" size_t rnerf_nerfmlp_save_bytes(int64_t rows, int backward) {
  const int64_t padded = (rows + 255) / 256 * 256;
  return save_payload_bytes(padded, bwd_two_planes(backward)) + SAVE_QUEUE_BYTES;
}

extern "C" int rnerf_nerfmlp_forward_train(const void* packed, int precision, const float* rows_pd, const float* rows_dr,
                                           const int32_t* node_of_sample, int32_t S, int32_t B, float* out_raw, void* save,
                                           int backward, int32_t max_workgroups, void* stream) {
  RNERF_CHECK_ARG(packed && rows_pd && rows_dr && out_raw && save, "rnerf_nerfmlp_forward_train: null pointer");
  RNERF_CHECK_ARG(max_workgroups >= 0, "rnerf_nerfmlp_forward_train: max_workgroups must be >= 0");
  RNERF_CHECK_ARG(bwd_ok(backward), "rnerf_nerfmlp_forward_train: unknown backward mode %d", backward);
  // (the bf16x3 forward is an inference-only precision: its 8-bit saved operands would cap every backward mode at bf16 accuracy)
  // F16: the single-pass training forward (one MFMA per product, the hi plane IS the operand) — with the single-plane backward modes only:
  // the north-star arithmetic as a labelled bench leg, never the default (11-bit products against the reference's fp32)
  // BF16X3 + backward BF16: the RANGE-SAFE training arithmetic (fp32's exponent range end to end: bf16 hi + lo products forward, the bf16 hi
  // plane saved as it is, bf16 gradients) — what a step is re-run in when the f16-based one met a row outside f16's range (train.py)
  RNERF_CHECK_ARG(train_combo_ok(precision, backward),
                  "rnerf_nerfmlp_forward_train: the training forward is built for precision f16x3, f16 with the single-plane backward modes, and bf16x3 with backward bf16");
  RNERF_CHECK_ARG(S >= 1 && B >= 1, "rnerf_nerfmlp_forward_train: need S >= 1 and B >= 1");
  RNERF_CHECK_ARG((((uintptr_t)packed | (uintptr_t)rows_pd | (uintptr_t)rows_dr | (uintptr_t)out_raw | (uintptr_t)save) & 15) == 0,
                  "rnerf_nerfmlp_forward_train: buffers must be 16-byte aligned");
  const long long total = (long long)S * B;
  hipStream_t st = (hipStream_t)stream;
  if (backward == RNERF_BWD_F16X2) return launch_fwd_mode<RNERF_PREC_F16X3, 0, 2>(packed, rows_pd, rows_dr, node_of_sample, B, total, out_raw, st, save, max_workgroups);
  if (backward == RNERF_BWD_F16X3_LO8) return launch_fwd_mode<RNERF_PREC_F16X3, 0, 3>(packed, rows_pd, rows_dr, node_of_sample, B, total, out_raw, st, save, max_workgroups);
  if (precision == RNERF_PREC_BF16X3) return launch_fwd_mode<RNERF_PREC_BF16X3, 0, 1>(packed, rows_pd, rows_dr, node_of_sample, B, total, out_raw, st, save, max_workgroups);
  if (precision == RNERF_PREC_F16) return launch_fwd_mode<RNERF_PREC_F16, 0, 1>(packed, rows_pd, rows_dr, node_of_sample, B, total, out_raw, st, save, max_workgroups);
  return launch_fwd_mode<RNERF_PREC_F16X3, 0, 1>(packed, rows_pd, rows_dr, node_of_sample, B, total, out_raw, st, save, max_workgroups);
}

extern "C" size_t rnerf_nerfmlp_bwd_packed_bytes(void) { return (size_t)kBwdBlocks * 2 * 1024; }
extern "C" size_t rnerf_nerfmlp_dy_bytes(int64_t rows, int backward) {
  const int64_t padded = (rows + 255) / 256 * 256;
  const int np = bwd_two_planes(backward) ? 2 : 1;
  return dy_plane_uint4(padded, np) * sizeof(uint4) + (backward == RNERF_BWD_BF16 ? 0 : ((size_t)padded + 4) * sizeof(float));
}

extern "C" int rnerf_nerfmlp_pack_bwd(const float* params, int backward, void* packed_bwd, void* stream) {
  RNERF_CHECK_ARG(params && packed_bwd, "rnerf_nerfmlp_pack_bwd: null pointer");
  RNERF_CHECK_ARG(bwd_ok(backward), "rnerf_nerfmlp_pack_bwd: unknown backward mode %d", backward);
  const int threads = kBwdBlocks * 64;
  if (backward == RNERF_BWD_BF16)
    hipLaunchKernelGGL(nerfmlp_pack_bwd_kernel<RNERF_PREC_BF16X3>, dim3((threads + 255) / 256), dim3(256), 0, (hipStream_t)stream, params, (char*)packed_bwd);
  else
    hipLaunchKernelGGL(nerfmlp_pack_bwd_kernel<RNERF_PREC_F16X3>, dim3((threads + 255) / 256), dim3(256), 0, (hipStream_t)stream, params, (char*)packed_bwd);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

// the dgrad's row-scale reference (m_ref, an atomicMax accumulator behind the row scales of the f16 modes' dY buffer; nullptr: none) — it
// must be zero when the kernel starts: launch_dgrad zeroes it unless the caller already has (nerfmlp_step_zero)
void* rnerf::nerfmlp_dgrad_scale_ref(int backward, void* dy, int64_t rows) {
  const long long R = (rows + 255) / 256 * 256;
  if (bwd_two_planes(backward)) return (char*)dy + dy_plane_uint4(R, Bwd<RNERF_BWD_F16X2>::NP) * sizeof(uint4) + (size_t)R * sizeof(float);
  if (backward == RNERF_BWD_F16) return (char*)dy + dy_plane_uint4(R, Bwd<RNERF_BWD_F16>::NP) * sizeof(uint4) + (size_t)R * sizeof(float);
  return nullptr;
}

template <int BWD>
static int launch_dgrad(const void* packed_bwd, const float* fwd_aux, const void* save, const float* d_raw, int64_t rows, void* dy, hipStream_t st,
                        bool zero_ref = true, bool allow_half = true) {
  using PB = Prec<Bwd<BWD>::PREC>;
  const int n_tiles = (int)((rows + 255) / 256);
  int dev = 0, cus = 0;
  RNERF_CHECK_HIP(hipGetDevice(&dev));
  RNERF_CHECK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const int grid = n_tiles < cus ? n_tiles : cus;
  const size_t lds = 2 * (size_t)PB::SLAB + 4 * 32768;
  static DeviceOnce attr_set;
  if (attr_set.need()) {
    RNERF_CHECK_HIP(hipFuncSetAttribute((const void*)nerfmlp_dgrad_kernel<BWD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set.set();
  }
  const long long R = (long long)n_tiles * 256;
  if (Bwd<BWD>::F16 && zero_ref) RNERF_CHECK_HIP(hipMemsetAsync(nerfmlp_dgrad_scale_ref(BWD == kBwdF16OnePass ? RNERF_BWD_F16 : BWD, dy, rows), 0, 4 * sizeof(float), st));
  // Few rows: 128-row tiles when they all fit one round (see launch_fwd_mode) — unless the caller runs another level's dgrad beside this one
  // (allow_half = false): two kernels that each own whole CUs then share the chip, and with twice the workgroups of half the work the
  // step measures the same or slower (512 rays, levels side by side: 2.05 -> 2.09 ms; alone, a 256-ray single-level step: 1.17 -> 1.12 ms).
  if constexpr (BWD == RNERF_BWD_F16X2 || BWD == RNERF_BWD_F16 || BWD == kBwdF16OnePass || BWD == RNERF_BWD_F16X3_LO8) {
    static const int half_lim = [] { const char* e = RNERF_ENV("RNERF_DGRAD_HALF_TILES"); return e ? atoi(e) : -1; }();      // 0: off, n: at most n tiles
    if (allow_half && half_lim != 0 && 2 * n_tiles <= (half_lim > 1 ? half_lim : cus)) {
      const size_t lds1 = 2 * (size_t)PB::SLAB;
      static DeviceOnce attr1_set;
      if (attr1_set.need()) {
        RNERF_CHECK_HIP(hipFuncSetAttribute((const void*)nerfmlp_dgrad_kernel<BWD, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1));
        attr1_set.set();
      }
      hipLaunchKernelGGL((nerfmlp_dgrad_kernel<BWD, true>), dim3(2 * n_tiles), dim3(256), lds1, st, (const char*)packed_bwd, fwd_aux, (const uint4*)save, R,
                         (const float4*)d_raw, (long long)rows, 2 * n_tiles, (uint4*)dy);
      RNERF_CHECK_LAUNCH();
      return RNERF_OK;
    }
  }
  hipLaunchKernelGGL(nerfmlp_dgrad_kernel<BWD>, dim3(grid), dim3(256), lds, st, (const char*)packed_bwd, fwd_aux, (const uint4*)save, R,
                     (const float4*)d_raw, (long long)rows, n_tiles, (uint4*)dy);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

namespace rnerf {
// zero_ref = false: the caller has zeroed nerfmlp_dgrad_scale_ref(backward, dy, rows) on `stream` already (nerfmlp_step_zero)
int nerfmlp_dgrad_impl(const void* packed_bwd, const void* packed_fwd, int fwd_precision, int backward, const void* save, const float* d_raw, int64_t rows,
                       void* dy, bool zero_ref, bool allow_half, hipStream_t st) {
  RNERF_CHECK_ARG(packed_bwd && packed_fwd && save && d_raw && dy, "rnerf_nerfmlp_dgrad: null pointer");
  RNERF_CHECK_ARG(train_combo_ok(fwd_precision, backward), "rnerf_nerfmlp_dgrad: forward precision must be f16x3 (f16 with a single-plane backward mode; bf16x3 with backward bf16)");
  RNERF_CHECK_ARG(bwd_ok(backward), "rnerf_nerfmlp_dgrad: unknown backward mode %d", backward);
  RNERF_CHECK_ARG(rows >= 1, "rnerf_nerfmlp_dgrad: rows must be >= 1");
  // the aux floats (biases, heads) sit behind the forward's operand stream, whose length depends on its precision
  const float* fwd_aux = (const float*)((const char*)packed_fwd + train_stream_bytes(fwd_precision));
  if (backward == RNERF_BWD_F16X2) return launch_dgrad<RNERF_BWD_F16X2>(packed_bwd, fwd_aux, save, d_raw, rows, dy, st, zero_ref, allow_half);
  if (backward == RNERF_BWD_F16X3_LO8) return launch_dgrad<RNERF_BWD_F16X3_LO8>(packed_bwd, fwd_aux, save, d_raw, rows, dy, st, zero_ref, allow_half);
  if (backward == RNERF_BWD_F16 && fwd_precision == RNERF_PREC_F16) return launch_dgrad<kBwdF16OnePass>(packed_bwd, fwd_aux, save, d_raw, rows, dy, st, zero_ref, allow_half);
  if (backward == RNERF_BWD_F16) return launch_dgrad<RNERF_BWD_F16>(packed_bwd, fwd_aux, save, d_raw, rows, dy, st, zero_ref, allow_half);
  return launch_dgrad<RNERF_BWD_BF16>(packed_bwd, fwd_aux, save, d_raw, rows, dy, st, zero_ref, allow_half);
}
}  // namespace rnerf

extern "C" int rnerf_nerfmlp_dgrad(const void* packed_bwd, const void* packed_fwd, int fwd_precision, int backward, const void* save,
                                   const float* d_raw, int64_t rows, void* dy, void* stream) {
  return nerfmlp_dgrad_impl(packed_bwd, packed_fwd, fwd_precision, backward, save, d_raw, rows, dy, true, true, (hipStream_t)stream);
}

// the wgrad jobs of one NerfMLP: {x slot base, x k-steps, dy slot base, dy k-steps, job, second-segment bases}
struct WgradPlan { int qx, KSx, qd, KSd; WgradJob job; int qx2, qd2, KSd2; };
static constexpr WgradJob job1(int dense, int xkind, int row_off, int dkind, int KT, int NT, int wb, int bias_sigma = 0) {
  return WgradJob{dense, xkind, row_off, dkind, KT, NT, wb, KT, 0, 0, NT, 0, 0, bias_sigma};
}
// 14 single-segment jobs: the bf16 body (MFMA transposition)
static const WgradPlan kWgradPlan[15] = {
    {SAVE_PE, 4, 0, 16, job1(0, 0, 0, 0, 2, 8, 1), 0, 0, 0},
    {SAVE_L1 + 0, 16, 16, 16, job1(1, 1, 0, 0, 8, 8, 1), 0, 0, 0},   {SAVE_L1 + 16, 16, 32, 16, job1(2, 1, 0, 0, 8, 8, 1), 0, 0, 0},
    {SAVE_L1 + 32, 16, 48, 16, job1(3, 1, 0, 0, 8, 8, 1), 0, 0, 0},  {SAVE_L1 + 48, 16, 64, 16, job1(4, 1, 0, 0, 8, 8, 1), 0, 0, 0},
    {SAVE_L1 + 64, 16, 80, 16, job1(5, 1, 0, 0, 8, 8, 1), 0, 0, 0},  {SAVE_PE, 4, 80, 16, job1(5, 0, 256, 0, 2, 8, 0), 0, 0, 0},
    {SAVE_L1 + 80, 16, 96, 16, job1(6, 1, 0, 0, 8, 8, 1), 0, 0, 0},  {SAVE_L1 + 96, 16, 112, 16, job1(7, 1, 0, 0, 8, 8, 1), 0, 0, 0},
    {SAVE_L1 + 112, 16, 128, 16, job1(9, 1, 0, 0, 8, 8, 1), 0, 0, 0}, {SAVE_L1 + 112, 16, DY_HEADS, 1, job1(8, 1, 0, 1, 8, 1, 1), 0, 0, 0},
    {SAVE_L1 + 128, 16, DY_L9, 8, job1(10, 1, 0, 0, 8, 4, 1), 0, 0, 0}, {SAVE_VIEW, 2, DY_L9, 8, job1(10, 2, 256, 0, 1, 4, 0), 0, 0, 0},
    {SAVE_RGBIN, 8, DY_HEADS, 1, job1(11, 1, 0, 2, 4, 1, 1), 0, 0, 0},
    {0, 0, 0, 0, job1(0, 0, 0, 0, 0, 0, 0), 0, 0, 0}};
// 11 jobs of the transpose-read kernel: an operand stream that two Dense blocks share is read once —
//   Dense_5 = [previous layer | position encoding] rows against dY_5 (10 k-tiles), Dense_10 = [bottleneck | view encoding] rows against
//   dY_9 (9 k-tiles), Dense_9 and the sigma head Dense_8 against the trunk output (8 + 1 n-tiles; the sigma bias comes from the rgb job)
static const WgradPlan kWgradPlanTr[12] = {
    {SAVE_PE, 4, 0, 16, job1(0, 0, 0, 0, 2, 8, 1), 0, 0, 0},
    {SAVE_L1 + 0, 16, 16, 16, job1(1, 1, 0, 0, 8, 8, 1), 0, 0, 0},   {SAVE_L1 + 16, 16, 32, 16, job1(2, 1, 0, 0, 8, 8, 1), 0, 0, 0},
    {SAVE_L1 + 32, 16, 48, 16, job1(3, 1, 0, 0, 8, 8, 1), 0, 0, 0},  {SAVE_L1 + 48, 16, 64, 16, job1(4, 1, 0, 0, 8, 8, 1), 0, 0, 0},
    {SAVE_L1 + 64, 20, 80, 16, WgradJob{5, 1, 0, 0, 10, 8, 1, /*KTa*/ 8, /*xkind2*/ 0, /*row_off2*/ 256, /*NTa*/ 8, 0, 0, 0}, SAVE_PE, 0, 0},
    {SAVE_L1 + 80, 16, 96, 16, job1(6, 1, 0, 0, 8, 8, 1), 0, 0, 0},  {SAVE_L1 + 96, 16, 112, 16, job1(7, 1, 0, 0, 8, 8, 1), 0, 0, 0},
    {SAVE_L1 + 112, 16, 128, 16, WgradJob{9, 1, 0, 0, 8, 9, 1, 8, 0, 0, /*NTa*/ 8, /*dense2*/ 8, /*dkind2*/ 1, 0}, 0, DY_HEADS, 1},
    {SAVE_L1 + 128, 18, DY_L9, 8, WgradJob{10, 1, 0, 0, 9, 4, 1, /*KTa*/ 8, /*xkind2*/ 2, /*row_off2*/ 256, 4, 0, 0, 0}, SAVE_VIEW, 0, 0},
    {SAVE_RGBIN, 8, DY_HEADS, 1, job1(11, 1, 0, 2, 4, 1, 1, /*bias_sigma*/ 1), 0, 0, 0},
    {0, 0, 0, 0, job1(0, 0, 0, 0, 0, 0, 0), 0, 0, 0}};

// legacy = the bf16 body (MFMA transposition): shares by MFMA count, 4 rounds of workgroups; otherwise the transpose-read bodies, paced
// by HBM: shares by bytes streamed per row, 2 rounds (measured with RNERF_WGRAD_TRACE: all jobs' workgroups finish within 10 %)
// mult: rounds of one-per-CU workgroups the rows are cut into (0: the default of the body — 4 legacy, 2 transposing)
static size_t build_wgrad_table(int cus, WgradTable& t, bool legacy, int mult = 0) {
  const WgradPlan* plan = legacy ? kWgradPlan : kWgradPlanTr;
  int n = 0;
  double cost[16], total = 0;
  for (; plan[n].KSx != 0; ++n) {
    const WgradJob& jb = plan[n].job;
    cost[n] = legacy ? 2.0 * jb.KT * jb.NT + 2 * (jb.KT + jb.NT) + 16 : jb.KT + jb.NT + 1;
    total += cost[n];
  }
  t.n = n;
  const int budget = (mult > 0 ? mult : (legacy ? 4 : 2)) * cus;
  size_t off = 0;
  int wg = 0;
  for (int i = 0; i < n; ++i) {
    const WgradPlan& p = plan[i];
    int share = (int)(budget * cost[i] / total + 0.5);
    if (share < 8) share = 8;
    t.qx[i] = p.qx; t.KSx[i] = p.KSx; t.qd[i] = p.qd; t.KSd[i] = p.KSd; t.job[i] = p.job;
    t.qx2[i] = p.qx2; t.qd2[i] = p.qd2; t.KSd2[i] = p.KSd2;
    t.wg0[i] = wg; wg += share;
    t.poff[i] = (long long)off; off += (size_t)share * p.job.KT * 32 * p.job.NT * 32;
    t.pboff[i] = (long long)off; off += (size_t)share * p.job.NT * 32;
  }
  t.wg0[n] = wg;
  return off;
}

static int device_cus() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  return cus;
}

// tr_small: the transposing body's table for a FEW rows (<= kWgradSmallRows: both levels of a 128-ray shard of the reference's default
// batch): one round of workgroups instead of two — every workgroup writes its whole partial dW block whatever its share of the rows, and
// with < 100 rows per workgroup that fixed cost is the kernel (128 rays: 1.29 -> 1.23 ms per step; from 32 768 rows on — the coarse level of
// a 512-ray batch — two rounds are faster: 2.14 against 2.18 ms in round 4; profiles/r04/small_batches.txt).  Smaller than `tr` in workgroups and partials:
// the workspace size is unchanged.
constexpr long long kWgradSmallRows = 24576;
struct WgradTables { WgradTable legacy, tr, tr_small; size_t partial_floats; int max_wgs; };
static const WgradTables& wgrad_tables() {
  // built once, by whichever host thread comes first (a function-local static's initialisation is thread-safe); sized by the compute units
  // of that thread's current device — every device a process drives is assumed to be the same part
  static const WgradTables tables = [] {
    WgradTables w;
    const size_t a = build_wgrad_table(device_cus(), w.legacy, true), b = build_wgrad_table(device_cus(), w.tr, false);
    const size_t s = build_wgrad_table(device_cus(), w.tr_small, false, 1);
    w.partial_floats = a > b ? a : b;
    if (s > w.partial_floats) w.partial_floats = s;
    w.max_wgs = w.legacy.wg0[w.legacy.n] > w.tr.wg0[w.tr.n] ? w.legacy.wg0[w.legacy.n] : w.tr.wg0[w.tr.n];
    if (w.tr_small.wg0[w.tr_small.n] > w.max_wgs) w.max_wgs = w.tr_small.wg0[w.tr_small.n];
    return w;
  }();
  return tables;
}

extern "C" size_t rnerf_nerfmlp_wgrad_workspace_bytes(void) {
  const WgradTables& w = wgrad_tables();
  return w.partial_floats * sizeof(float) + (size_t)w.max_wgs * 2 * sizeof(long long);       // + the RNERF_WGRAD_TRACE slots
}

// host side of the transposing wgrad for one operand format; launch returns where the dgrad left m_ref (behind the row scales)
template <class Planes> struct WgradTrHost {
  static hipError_t allow_lds() {
    return hipFuncSetAttribute((const void*)nerfmlp_wgrad_tr_kernel<Planes>, hipFuncAttributeMaxDynamicSharedMemorySize, Planes::lds_bytes());
  }
  static const float* launch(const WgradTable& tab, hipStream_t st, const void* save, const void* dy, long long R, void* workspace, long long* trace) {
    hipLaunchKernelGGL(nerfmlp_wgrad_tr_kernel<Planes>, dim3(tab.wg0[tab.n]), dim3(512), Planes::lds_bytes(), st, (const uint4*)save, (const uint4*)dy, R,
                       (float*)workspace, tab, trace);
    return (const float*)((const uint4*)dy + dy_plane_uint4(R, Planes::NPLANES)) + R;
  }
};

extern "C" int rnerf_nerfmlp_wgrad(int fwd_precision, int backward, const void* save, const void* dy, int64_t rows, float* grads, void* workspace,
                                   void* stream) {
  RNERF_CHECK_ARG(save && dy && grads && workspace, "rnerf_nerfmlp_wgrad: null pointer");
  RNERF_CHECK_ARG(train_combo_ok(fwd_precision, backward), "rnerf_nerfmlp_wgrad: forward precision must be f16x3 (f16 with a single-plane backward mode; bf16x3 with backward bf16)");
  RNERF_CHECK_ARG(bwd_ok(backward), "rnerf_nerfmlp_wgrad: unknown backward mode %d", backward);
  RNERF_CHECK_ARG(rows >= 1, "rnerf_nerfmlp_wgrad: rows must be >= 1");
  const WgradTables& w = wgrad_tables();
  static DeviceOnce ready;
  if (ready.need()) {
    RNERF_CHECK_HIP(hipFuncSetAttribute((const void*)nerfmlp_wgrad_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072));
    RNERF_CHECK_HIP(hipFuncSetAttribute((const void*)nerfmlp_wgrad_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 131072));
    RNERF_CHECK_HIP(WgradTrHost<F16Planes<1>>::allow_lds());
    RNERF_CHECK_HIP(WgradTrHost<F16Planes<2>>::allow_lds());
    RNERF_CHECK_HIP(WgradTrHost<Lo8Planes>::allow_lds());
    ready.set();
  }
  const long long R = (rows + 255) / 256 * 256;
  hipStream_t st = (hipStream_t)stream;
  const float* out_scale = nullptr;
  // RNERF_WGRAD_TRACE=1 (profiling aid): per-workgroup start / end times behind the partials -> per-job spans on stderr (synchronises)
  static const bool tracing = RNERF_ENV("RNERF_WGRAD_TRACE") != nullptr;
  long long* trace = tracing ? (long long*)((char*)workspace + w.partial_floats * sizeof(float)) : nullptr;
  const WgradTable& tab = backward == RNERF_BWD_BF16 ? w.legacy : (rows <= kWgradSmallRows ? w.tr_small : w.tr);
  if (backward == RNERF_BWD_BF16) {
    const int n_chunks = (int)((rows + 127) / 128);
    if (fwd_precision == RNERF_PREC_BF16X3)      // the range-safe step: the saved plane is bf16 already
      hipLaunchKernelGGL(nerfmlp_wgrad_kernel<false>, dim3(tab.wg0[tab.n]), dim3(512), 131072, st, (const uint4*)save, (const uint4*)dy, R,
                         (long long)rows, n_chunks, (float*)workspace, tab);
    else
      hipLaunchKernelGGL(nerfmlp_wgrad_kernel<true>, dim3(tab.wg0[tab.n]), dim3(512), 131072, st, (const uint4*)save, (const uint4*)dy, R,
                         (long long)rows, n_chunks, (float*)workspace, tab);
  } else if (backward == RNERF_BWD_F16) {
    out_scale = WgradTrHost<F16Planes<1>>::launch(tab, st, save, dy, R, workspace, trace);
  } else if (backward == RNERF_BWD_F16X3_LO8) {
    out_scale = WgradTrHost<Lo8Planes>::launch(tab, st, save, dy, R, workspace, trace);
  } else {
    out_scale = WgradTrHost<F16Planes<2>>::launch(tab, st, save, dy, R, workspace, trace);
  }
  int max_elems = 0;
  for (int j = 0; j < tab.n; ++j) max_elems = tab.job[j].KT * tab.job[j].NT * 1024 > max_elems ? tab.job[j].KT * tab.job[j].NT * 1024 : max_elems;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((max_elems + 255) / 256, tab.n), dim3(256), 0, st, (const float*)workspace, tab, grads, out_scale);
  RNERF_CHECK_LAUNCH();
  if (trace && backward != RNERF_BWD_BF16) {
    const int n_wg = tab.wg0[tab.n];
    std::vector<long long> h(2 * (size_t)n_wg);
    RNERF_CHECK_HIP(hipStreamSynchronize(st));
    RNERF_CHECK_HIP(hipMemcpy(h.data(), trace, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
    long long t0 = h[0];
    for (int i = 0; i < n_wg; ++i) t0 = h[2 * i] < t0 ? h[2 * i] : t0;
    for (int j = 0; j < tab.n; ++j) {
      long long a = -1, b = 0; double busy = 0;
      for (int i = tab.wg0[j]; i < tab.wg0[j + 1]; ++i) { a = (a < 0 || h[2 * i] < a) ? h[2 * i] : a; b = h[2 * i + 1] > b ? h[2 * i + 1] : b; busy += (double)(h[2 * i + 1] - h[2 * i]); }
      fprintf(stderr, "[wgrad trace] job %2d (KT %d NT %d) wgs %4d  first start %9lld  last end %9lld  mean wg ticks (100 MHz) %7.0f\n", j, tab.job[j].KT, tab.job[j].NT,
              tab.wg0[j + 1] - tab.wg0[j], a - t0, b - t0, busy / (tab.wg0[j + 1] - tab.wg0[j]));
    }
  }
  return RNERF_OK;
}

extern "C" int rnerf_nerfmlp_input_grad(const float* params, int backward, const void* dy, const float* rows_pd, const float* rows_dr,
                                        const int32_t* node_of_sample, int32_t S, int32_t B, float* d_pos4, float* d_dir4, void* stream) {
  RNERF_CHECK_ARG(params && dy && rows_pd && rows_dr && d_pos4 && d_dir4, "rnerf_nerfmlp_input_grad: null pointer");
  RNERF_CHECK_ARG(backward == RNERF_BWD_F16 || backward == RNERF_BWD_F16X2 || backward == RNERF_BWD_F16X3_LO8, "rnerf_nerfmlp_input_grad: needs the row-normalised f16 backward modes");
  RNERF_CHECK_ARG(S >= 1 && B >= 1, "rnerf_nerfmlp_input_grad: need S >= 1 and B >= 1");
  const long long rows = (long long)S * B;
  const long long R = (rows + 255) / 256 * 256;
  const unsigned grid = (unsigned)((rows + 31) / 32);
  hipStream_t st = (hipStream_t)stream;
  if (backward == RNERF_BWD_F16X3_LO8)
    hipLaunchKernelGGL(nerfmlp_input_grad_kernel<3>, dim3(grid), dim3(64), 0, st, params, (const uint4*)dy, R, (const float4*)rows_pd, (const float4*)rows_dr,
                       node_of_sample, B, rows, (float4*)d_pos4, (float4*)d_dir4);
  else if (backward == RNERF_BWD_F16X2)
    hipLaunchKernelGGL(nerfmlp_input_grad_kernel<2>, dim3(grid), dim3(64), 0, st, params, (const uint4*)dy, R, (const float4*)rows_pd, (const float4*)rows_dr,
                       node_of_sample, B, rows, (float4*)d_pos4, (float4*)d_dir4);
  else
    hipLaunchKernelGGL(nerfmlp_input_grad_kernel<1>, dim3(grid), dim3(64), 0, st, params, (const uint4*)dy, R, (const float4*)rows_pd, (const float4*)rows_dr,
                       node_of_sample, B, rows, (float4*)d_pos4, (float4*)d_dir4);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}
