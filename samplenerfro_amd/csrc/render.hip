// Compositing (V1) and hierarchical resampling along the bent path (S1/S2).
// Reference: rnerf/models.py:334-349 (activations + call), rnerf/model_utils.py:247-309 (volumetric_rendering),
// :312-374 (sorted_piecewise_constant_pdf), :377-435 (sample_pdf).
//
// Both kernels are one-lane-per-ray sequential walks over sample-major arrays: every per-step load/store of a wave is
// one contiguous segment, no scan or sort network is needed (the coarse depths, the inverse-CDF samples and the path
// node depths are all already sorted, so sort + searchsorted collapse into one three-way merge walk).
#include "common.h"

#include <float.h>

namespace rnerf {

__device__ __forceinline__ float sigmoidf_ref(float x) { return fdiv(1.0f, fadd(1.0f, expf(-x))); }
// jax.nn.softplus = logaddexp(x, 0) = max(x,0) + log1p(exp(-|x|))
__device__ __forceinline__ float softplusf_ref(float x) { return fadd(fmaxf(x, 0.f), log1pf(expf(-fabsf(x)))); }

// L consecutive lanes per ray (L = 4: a DPP quad; 16 or 64: broadcasts through ds_bpermute): lane q owns samples L j + q.  Everything that
// does not depend on the running optical depth (activations: 3 sigmoids + softplus, segment length, alpha — nearly all of the
// instructions) is computed by the L lanes at once; the recurrence itself — cum += dd and the five ordered accumulations — is replayed in
// SAMPLE ORDER through lane broadcasts, so every sum is built by the same sequence of individually rounded additions as a one-lane loop
// (and the reference's cumsum order) whatever L: the kernels give the same bits for every L (tests/test_gpu_parity.py).  The kernels are
// bound by the LATENCY of a ray's chain of groups (S / L iterations of ~250 dependent-ish instructions with one wave per SIMD): the
// launcher picks the widest L that still leaves every SIMD a few waves (round 4: 4 lanes per ray at 4096 rays x 128 samples were 256 waves
// on 1024 SIMDs: 36 us forward, 57 us backward; 128 rays x 192 samples 47 / 76 us).
template <int L>
__device__ __forceinline__ float ray_bcast(float v, int i) {      // value of lane i of this lane's group of L
  if constexpr (L == 4) return i == 0 ? quad_bcast<0>(v) : (i == 1 ? quad_bcast<1>(v) : (i == 2 ? quad_bcast<2>(v) : quad_bcast<3>(v)));
  else return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((int)((((threadIdx.x & 63) & ~(L - 1)) + i) << 2), __builtin_bit_cast(int, v)));
}
template <int L>
__device__ __forceinline__ int ray_bcast_i(int v, int i) { return __builtin_bit_cast(int, ray_bcast<L>(__builtin_bit_cast(float, v), i)); }
template <int L>
__device__ __forceinline__ float ray_next(float v) {              // value of the NEXT lane of the group (the last lane's is unused)
  if constexpr (L == 4) return quad_next(v);
  else return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((int)(((threadIdx.x & 63) + 1) & 63) << 2, __builtin_bit_cast(int, v)));
}

template <int L>
__global__ void __launch_bounds__(64) composite_kernel(const float4* __restrict__ raw, const float4* __restrict__ rows_pd,
                                                       const float4* __restrict__ rows_dr,
                                                       const int* __restrict__ node_of_sample, int S, int B,
                                                       const float* __restrict__ bkgd, int white_bkgd, float pad_scale,
                                                       float pad, float sigma_bias, float* __restrict__ rgb_out,
                                                       float* __restrict__ dist_out, float* __restrict__ acc_out,
                                                       float* __restrict__ trans_out, float* __restrict__ trans_bkgd_out,
                                                       float* __restrict__ weights, float* __restrict__ alpha_out,
                                                       int mask_mode, float bx0, float by0, float bz0, float bx1, float by1, float bz1) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int q = gid & (L - 1);
  int r = gid / L;
  const bool live = r < B;
  if (!live) r = B - 1;            // surplus groups replay the last ray (the broadcasts need whole groups); their stores are suppressed
  auto rec = [&](int s) -> size_t { return (size_t)(node_of_sample ? node_of_sample[s] : s) * B + r; };
  const int G = (S + L - 1) / L;
  // mask_bbox = (cumsum(inside[::-1]) > 0)[::-1] (rnerf/models.py:498-503): 1 up to and including the LAST sample inside the
  // box; mask_mode 1 uses it, mask_mode 2 uses 1 - mask (:505-523).  mask_mode 3 = use_mask_bbox (:261-271,398-408): the plain per-sample
  // test "this sample is inside the box".
  int last_in = -1;
  if (mask_mode == 1 || mask_mode == 2) {
    for (int j = G - 1; j >= 0; --j) {
      const int s = L * j + q;
      if (s < S) {
        const float4 p = rows_pd[rec(s)];
        if (p.x >= bx0 && p.x <= bx1 && p.y >= by0 && p.y <= by1 && p.z >= bz0 && p.z <= bz1) { last_in = s; break; }
      }
    }
    int mx = ray_bcast_i<L>(last_in, 0);
#pragma unroll
    for (int i = 1; i < L; ++i) mx = max(mx, ray_bcast_i<L>(last_in, i));
    last_in = mx;
  }
  float cum = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, acc = 0.f, wt = 0.f;
  const float t0 = rows_pd[rec(0)].w;
  const float t_last = rows_pd[rec(S - 1)].w;
  struct Rec { float4 d, rw; float t; float in; };
  auto load = [&](int j) -> Rec {
    int s = L * j + q;
    if (s > S - 1) s = S - 1;
    const size_t o = rec(s);
    Rec x;
    const float4 p = rows_pd[o];
    x.d = rows_dr[o]; x.rw = raw[(size_t)s * B + r]; x.t = p.w;
    x.in = (mask_mode != 3 || (p.x >= bx0 && p.x <= bx1 && p.y >= by0 && p.y <= by1 && p.z >= bz0 && p.z <= bz1)) ? 1.0f : 0.0f;
    return x;
  };
  // ordered accumulation of the L lanes' products: (((a + p0) + p1) + p2) + ...
  auto acc4 = [&](float a, float p) -> float {
#pragma unroll
    for (int i = 0; i < L; ++i) a = fadd(a, ray_bcast<L>(p, i));
    return a;
  };
  Rec cur = load(0);
  for (int j = 0; j < G; ++j) {
    const Rec nxt = load(j + 1 < G ? j + 1 : j);                // the next group's records are in flight during this group's arithmetic
    const int s = L * j + q;
    const bool valid = s < S;
    const float4 d = cur.d, rw = cur.rw;
    const float t_cur = cur.t;
    const float t_up = ray_next<L>(t_cur), t_grp = ray_bcast<L>(nxt.t, 0);
    const float t_next = q < L - 1 ? t_up : t_grp;
    const float tdist = (s + 1 < S) ? fsub(t_next, t_cur) : 1e-3f;   // model_utils.py:265-268
    const float nrm = fsqrt(fadd(fadd(fmul(d.x, d.x), fmul(d.y, d.y)), fmul(d.z, d.z)));
    const float delta = fmul(tdist, nrm);                    // :270
    const float sigma = softplusf_ref(fadd(rw.w, sigma_bias));   // models.py:338
    const float cr = fsub(fmul(sigmoidf_ref(rw.x), pad_scale), pad);   // models.py:334-335
    const float cg = fsub(fmul(sigmoidf_ref(rw.y), pad_scale), pad);
    const float cb = fsub(fmul(sigmoidf_ref(rw.z), pad_scale), pad);
    float dd = fmul(sigma, delta);                           // :272
    if (mask_mode == 3) dd = fmul(dd, cur.in);
    else if (mask_mode != 0) dd = fmul(dd, ((s <= last_in) == (mask_mode == 1)) ? 1.0f : 0.0f);   // density_delta *= mask_bbox (:275-276)
    if (!valid) dd = 0.f;                                    // padding lanes of the last group: alpha = 0, weight = 0
    const float a = fsub(1.0f, expf(-dd));                   // :285
    // optical depth before each of the group's samples, in order
    float my_cum = cum;
#pragma unroll
    for (int i = 0; i < L; ++i) { if (q == i) my_cum = cum; cum = fadd(cum, ray_bcast<L>(dd, i)); }
    const float T = expf(-my_cum);                           // :286-289
    const float w = fmul(a, T);                              // :296
    sr = acc4(sr, fmul(w, cr)); sg = acc4(sg, fmul(w, cg)); sb = acc4(sb, fmul(w, cb));
    acc = acc4(acc, w);
    wt = acc4(wt, fmul(w, t_cur));
    if (valid && live) {
      if (weights) weights[(size_t)s * B + r] = w;
      if (alpha_out) alpha_out[(size_t)s * B + r] = a;
    }
    cur = nxt;
  }
  if (q != 0 || !live) return;
  const float Tl = expf(-cum);
  float br = 1.f, bg = 1.f, bb = 1.f;                       // rgb_bkgd=None -> ones (:301)
  if (bkgd) {
    br = bkgd[3 * r]; bg = bkgd[3 * r + 1]; bb = bkgd[3 * r + 2];
    sr = fadd(sr, fmul(Tl, br)); sg = fadd(sg, fmul(Tl, bg)); sb = fadd(sb, fmul(Tl, bb));   // :298-299
  }
  float dist = fdiv(wt, acc);                                // :303
  // jnp.nan_to_num(distance, jnp.inf): 2nd positional is `copy` -> NaN->0, +-inf -> +-FLT_MAX (:304)
  if (dist != dist) dist = 0.f;
  else if (dist > FLT_MAX) dist = FLT_MAX;
  else if (dist < -FLT_MAX) dist = -FLT_MAX;
  dist = fminf(fmaxf(dist, t0), t_last);
  if (white_bkgd) { const float q = fsub(1.0f, acc); sr = fadd(sr, q); sg = fadd(sg, q); sb = fadd(sb, q); }   // :307-308
  rgb_out[3 * r] = sr; rgb_out[3 * r + 1] = sg; rgb_out[3 * r + 2] = sb;
  dist_out[r] = dist;
  acc_out[r] = acc;
  trans_out[r] = Tl;
  trans_bkgd_out[3 * r] = fmul(Tl, br); trans_bkgd_out[3 * r + 1] = fmul(Tl, bg); trans_bkgd_out[3 * r + 2] = fmul(Tl, bb);
}

// ---- T1 (first half): loss reductions and the backward of activations + volumetric_rendering ----------------------------------
// train.py:89-92,105: loss = mean((rgb_f - pix)^2) + mean((rgb_c - pix)^2)
//                            + bg_weight * 1[alpha>0] * sum(mask * |trans_rgb_bkgd_f - pix|) / (sum(mask) + 1),  mask = trans_f > 0.5
// sums[0] = sum (rgb_f-pix)^2, sums[1] = sum (rgb_c-pix)^2, sums[2] = sum mask*|tb_f-pix|, sums[3] = sum mask (rays)
// ONE workgroup, fixed reduction tree: the four sums are the same bits on every run (they used to be float atomics over 16 workgroups), and
// the kernel writes them outright — no memset launch ahead of it.
__global__ void __launch_bounds__(1024) loss_reduce_kernel(const float* __restrict__ rgb_c, const float* __restrict__ rgb_f,
                                                           const float* __restrict__ trans_f, const float* __restrict__ tb_f,
                                                           const float* __restrict__ pix, int B, float* __restrict__ sums) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int r = threadIdx.x; r < B; r += blockDim.x) {
    const float m = trans_f[r] > 0.5f ? 1.f : 0.f;
    a3 += m;
    for (int c = 0; c < 3; ++c) {
      const float p = pix[3 * r + c];
      const float df = rgb_f[3 * r + c] - p;
      a0 += df * df;
      if (rgb_c) { const float dc = rgb_c[3 * r + c] - p; a1 += dc * dc; }
      a2 += m * fabsf(tb_f[3 * r + c] - p);
    }
  }
  for (int o = 32; o > 0; o >>= 1) { a0 += __shfl_down(a0, o); a1 += __shfl_down(a1, o); a2 += __shfl_down(a2, o); a3 += __shfl_down(a3, o); }
  __shared__ float red[16][4];
  if ((threadIdx.x & 63) == 0) { float* q = red[threadIdx.x >> 6]; q[0] = a0; q[1] = a1; q[2] = a2; q[3] = a3; }
  __syncthreads();
  if (threadIdx.x < 4) {
    float s = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w][threadIdx.x];
    sums[threadIdx.x] = s;
  }
}

// Backward of one level: d loss / d raw (rgb, sigma) per sample and d loss / d bkgd per ray.
//   C = sum_s w_s c_s + T_S bk,  w_s = (1 - exp(-dd_s)) T_s,  T_s = exp(-sum_{j<s} dd_j),  dd_s = softplus(raw_sigma + b) * delta_s
//   d/d dd_s = (gC . c_s) T_{s+1} - sum_{j>s} (gC . c_j) w_j - G_T T_S,   G_T = gC . bk + gTB . bk     (model_utils.py:285-299,309)
//   gC = 2 (C - pix) / (3B);  gTB = bg_scale * mask * sign(T_S bk - pix) / (sum(mask) + 1)  (fine level only; bk is stop_gradient there)
// One lane per ray: a forward sweep for the total optical depth, then a reverse sweep that recomputes T on the way back.
template <int L>
__global__ void __launch_bounds__(64) composite_bwd_kernel(const float4* __restrict__ raw, const float4* __restrict__ rows_pd,
                                                           const float4* __restrict__ rows_dr, const int* __restrict__ node_of_sample,
                                                           int S, int B, const float* __restrict__ bkgd, float pad_scale, float pad,
                                                           float sigma_bias, const float* __restrict__ rgb, const float* __restrict__ pix,
                                                           const float* __restrict__ trans, const float* __restrict__ tb,
                                                           const float* __restrict__ sums, float mse_scale, float bg_scale,
                                                           float4* __restrict__ d_raw, float* __restrict__ d_bkgd, int accumulate_bkgd,
                                                           int mask_mode, float bx0, float by0, float bz0, float bx1, float by1, float bz1,
                                                           int white_bkgd) {
  // mask_mode: 0 = none; 1 = the bd_cut_dist pair (rnerf/models.py:479-524); 3 = use_mask_bbox (:261-271,398-408): density_delta *= 1[sample
  // inside the box] in this level's rendering — the mask multiplies the segment length, so dd and every gradient through it carry it
  const bool bd_cut = mask_mode == 1;
  // L lanes per ray, lane q owns samples L j + q (see composite_kernel): the ordered chains run through lane broadcasts
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int q = gid & (L - 1);
  int r = gid / L;
  const bool live = r < B;
  if (!live) r = B - 1;
  const int G = (S + L - 1) / L;
  auto rec = [&](int s) -> size_t { return (size_t)(node_of_sample ? node_of_sample[s] : s) * B + r; };
  const float wb1 = white_bkgd ? 1.0f : 0.0f;       // comp_rgb += 1 - acc (model_utils.py:307-308): every weight also carries -1 per channel
  float gC[3], bk[3], gTB[3] = {0.f, 0.f, 0.f};
  float GT = 0.f;
  // bd_cut (rnerf/models.py:479-524): the loss_bg pair is trans_A = exp(-sum_{s <= L} dd_s) (L = last sample inside the box) and
  // trans_A * C_B with C_B = composite of the samples s > L over bkgd (NOT stop-gradient there: rgb_bkgd=bkgd, :514-523).
  int last_in = -1;
  float gA = 0.f, gCB[3] = {0.f, 0.f, 0.f}, GTB = 0.f;
  for (int c = 0; c < 3; ++c) {
    bk[c] = bkgd[3 * r + c];
    gC[c] = mse_scale * (rgb[3 * r + c] - pix[3 * r + c]);
    GT += gC[c] * bk[c];
  }
  if (bd_cut) {
    for (int j = G - 1; j >= 0; --j) {
      const int s = L * j + q;
      if (s < S) {
        const float4 p = rows_pd[rec(s)];
        if (p.x >= bx0 && p.x <= bx1 && p.y >= by0 && p.y <= by1 && p.z >= bz0 && p.z <= bz1) { last_in = s; break; }
      }
    }
    int mx = ray_bcast_i<L>(last_in, 0);
#pragma unroll
    for (int i = 1; i < L; ++i) mx = max(mx, ray_bcast_i<L>(last_in, i));
    last_in = mx;
  }
  float trA = 1.f;
  if (bg_scale != 0.f && trans[r] > 0.5f) {
    const float inv = bg_scale / (sums[3] + 1.0f);
    trA = trans[r];
    for (int c = 0; c < 3; ++c) {
      const float d = tb[3 * r + c] - pix[3 * r + c];
      gTB[c] = d > 0.f ? inv : (d < 0.f ? -inv : 0.f);
      if (!bd_cut) GT += gTB[c] * bk[c];                   // d (trans * stop_gradient(bkgd)) / d trans
      else {
        gA += gTB[c] * (tb[3 * r + c] / trA);                // d / d trans_A  (C_B = trans_rgb_bkgd / trans_A, trans_A > 0.5 here)
        gCB[c] = gTB[c] * trA;                               // d / d C_B
        GTB += gCB[c] * bk[c];
      }
    }
  }
  struct Rec { float4 d, rw; float t; float in; };
  auto load = [&](int j) -> Rec {
    int s = L * j + q;
    if (s > S - 1) s = S - 1;
    const size_t o = rec(s);
    Rec x;
    const float4 p = rows_pd[o];
    x.d = rows_dr[o]; x.rw = raw[(size_t)s * B + r]; x.t = p.w;
    x.in = (mask_mode != 3 || (p.x >= bx0 && p.x <= bx1 && p.y >= by0 && p.y <= by1 && p.z >= bz0 && p.z <= bz1)) ? 1.0f : 0.0f;
    return x;
  };
  // dd of this lane's sample (0 for the padding lanes of the last group), d softplus/dx and the segment length
  auto dd_of = [&](const Rec& c, int s, float t_next, float& sg_out, float& delta_out) -> float {
    const float tdist = (s + 1 < S) ? fsub(t_next, c.t) : 1e-3f;
    const float nrm = fsqrt(fadd(fadd(fmul(c.d.x, c.d.x), fmul(c.d.y, c.d.y)), fmul(c.d.z, c.d.z)));
    delta_out = fmul(fmul(tdist, nrm), c.in);              // (use_mask_bbox: a sample outside the box has no density_delta and no gradient)
    const float x = fadd(c.rw.w, sigma_bias);
    sg_out = fdiv(1.0f, fadd(1.0f, expf(-x)));             // d softplus / dx
    return s < S ? fmul(softplusf_ref(x), delta_out) : 0.f;
  };
  // forward sweep: total optical depth, summed in sample order
  float cum = 0.f, cumB = 0.f;
  {
    Rec cur = load(0);
    for (int j = 0; j < G; ++j) {
      const Rec nxt = load(j + 1 < G ? j + 1 : j);
      const int s = L * j + q;
      const float t_up = ray_next<L>(cur.t), t_grp = ray_bcast<L>(nxt.t, 0);
      float a, b2;
      const float dd = dd_of(cur, s, q < L - 1 ? t_up : t_grp, a, b2);
      const float ddB = (bd_cut && s > last_in) ? dd : 0.f;
#pragma unroll
      for (int i = 0; i < L; ++i) cum = fadd(cum, ray_bcast<L>(dd, i));
      if (bd_cut) {
#pragma unroll
        for (int i = 0; i < L; ++i) cumB = fadd(cumB, ray_bcast<L>(ddB, i));
      }
      cur = nxt;
    }
  }
  const float TS = expf(-cum), TBS = expf(-cumB);
  float suffix = 0.f;          // sum_{j>s} (gC . c_j) w_j
  float cum_after = cum;
  float suffixB = 0.f, cumB_after = cumB;
  // a chain that runs from the group's LAST sample to its first: x3 = v - b3, x2 = x3 - b2, ...; `mine` = value before this lane's
  // own term (lane 3: v), `out` = value after all four
  auto chain_sub = [&](float v, float term, float& mine_after, float& mine_before) -> float {
    mine_after = v; mine_before = v;
#pragma unroll
    for (int i = L - 1; i >= 0; --i) {
      if (q == i) mine_after = v;
      v = fsub(v, ray_bcast<L>(term, i));
      if (q == i) mine_before = v;
    }
    return v;
  };
  auto chain_add = [&](float v, float term, float& mine) -> float {       // suffix sums: the last lane sees v, the one before it v + p_last, ...
    mine = v;
#pragma unroll
    for (int i = L - 1; i >= 0; --i) {
      if (q == i) mine = v;
      v = v + ray_bcast<L>(term, i);
    }
    return v;
  };
  {
    Rec cur = load(G - 1);
    float t_first_of_next = 0.f;                            // depth of sample 4(j+1): lane 0 of the group processed before
    for (int j = G - 1; j >= 0; --j) {
      const Rec nxt = load(j > 0 ? j - 1 : 0);
      const int s = L * j + q;
      const bool valid = s < S;
      const float t_up = ray_next<L>(cur.t);
      float sgp, delta;
      const float dd = dd_of(cur, s, q < L - 1 ? t_up : t_first_of_next, sgp, delta);
      t_first_of_next = ray_bcast<L>(cur.t, 0);
      float my_after, my_before;
      cum_after = chain_sub(cum_after, dd, my_after, my_before);
      const float T_next = expf(-my_after);
      const float T_s = (s == 0) ? 1.0f : expf(-my_before);
      const float a1 = fsub(1.0f, expf(-dd));
      const float w = fmul(a1, T_s);
      const float4 rw = cur.rw;
      const float sr = sigmoidf_ref(rw.x), sgn = sigmoidf_ref(rw.y), sb = sigmoidf_ref(rw.z);
      const float cr = sr * pad_scale - pad, cg = sgn * pad_scale - pad, cb = sb * pad_scale - pad;
      const float gcc = gC[0] * (cr - wb1) + gC[1] * (cg - wb1) + gC[2] * (cb - wb1);
      float my_suffix;
      suffix = chain_add(suffix, valid ? gcc * w : 0.f, my_suffix);
      float g_dd = gcc * T_next - my_suffix - GT * TS;
      float gr = gC[0] * w, gg = gC[1] * w, gb = gC[2] * w;
      if (bd_cut) {
        const bool behind = s > last_in;                       // the chain behind the box
        float myB_after, myB_before, my_suffixB;
        cumB_after = chain_sub(cumB_after, (behind && valid) ? dd : 0.f, myB_after, myB_before);
        const float TB_next = expf(-myB_after);
        const float TB_s = (s == last_in + 1) ? 1.0f : expf(-myB_before);
        const float wB = fmul(a1, TB_s);
        const float gccB = gCB[0] * cr + gCB[1] * cg + gCB[2] * cb;
        suffixB = chain_add(suffixB, (behind && valid) ? gccB * wB : 0.f, my_suffixB);
        if (behind) {
          g_dd += gccB * TB_next - my_suffixB - GTB * TBS;
          gr += gCB[0] * wB; gg += gCB[1] * wB; gb += gCB[2] * wB;
        } else {
          g_dd -= gA * trA;                                    // d trans_A / d dd_s = -trans_A
        }
      }
      if (valid && live) {
        float4 o;
        o.x = gr * pad_scale * sr * (1.0f - sr);
        o.y = gg * pad_scale * sgn * (1.0f - sgn);
        o.z = gb * pad_scale * sb * (1.0f - sb);
        o.w = g_dd * delta * sgp;
        d_raw[(size_t)s * B + r] = o;
      }
      cur = nxt;
    }
  }
  if (q != 0 || !live) return;
  for (int c = 0; c < 3; ++c) {
    const float g = gC[c] * TS + (bd_cut ? gCB[c] * TBS : 0.f);
    if (accumulate_bkgd) d_bkgd[3 * r + c] += g; else d_bkgd[3 * r + c] = g;
  }
}

// Resampling = two kernels.
//  (1) resample_depths_kernel, four lanes per ray: sorted_piecewise_constant_pdf + jnp.sort(concat(coarse, fine)).
//        bins  = mids of the S coarse depths (S-1 values), weights = w[1..S-2] (S-2 values)         models.py:371-374
//        cdf   = [0, min(1, cumsum(pdf[:-1])), 1]  (S-1 values)                                      model_utils.py:335-340
//        i*(u) = #(cdf <= u) - 1 ; sample = bins[i*] + clip((u-cdf[i*])/(cdf[i*+1]-cdf[i*]),0,1)*(bins[i*+1]-bins[i*])
//      u must be non-decreasing along the sample axis of each ray (true for both branches at :345-356), which makes the
//      samples non-decreasing, so the sort (:405) is a two-way merge of two sorted sequences.  The ray's coarse depths
//      and weights are staged in LDS; the two prefix chains run in index order through quad broadcasts, the inverse-CDF
//      lookups and the merge ranks are binary searches (independent per element).
//  (2) resample_gather_kernel, one lane per (sample, ray): searchsorted(z_vals, z, 'left') into the N node depths
//      (:415-421) from an arithmetic guess + gallop + bisection (node depths are near + ~k*step), then the gather
//      pos = path_pos[idx] + dir[idx]*(z - z_vals[idx]) (:423-427).  Neighbouring lanes = neighbouring rays at the same
//      sample index, whose node indices nearly coincide, so the probes and gathers of a wave are near-contiguous.
template <int RPB>      // rays per 64-lane block: 16 (a quad per ray), 4 (16 lanes per ray) or 1 (the whole wave): few rays, or S and F beyond the LDS staging at 16
__global__ void __launch_bounds__(64) resample_depths_kernel(const float4* __restrict__ path_pd, int B,
                                                             const int* __restrict__ jitter, int S,
                                                             const float* __restrict__ weights, const float* __restrict__ u,
                                                             int u_per_ray, int F, float* __restrict__ zbuf) {
  // L = 64 / RPB lanes per ray (like the compositing kernels: the work is a per-ray chain of dependent LDS round trips, so few rays are
  // given more lanes each).  LDS arrays are [index][RPB rays] (a ray's lanes hit consecutive banks):
  //   tcA[S] coarse depths, wA[S] coarse weights -> pdf terms, cdfA[S-1], zfA[F] fine depths, mgA[S+F] merged depths.
  // Only two chains are inherently sequential — the weight sum and the cdf prefix sum; both are replayed in index order through
  // quad broadcasts (same individually rounded additions as a one-lane loop).  The inverse-CDF lookups and the merge of the two
  // sorted lists are independent per element: binary searches instead of the serial (and lane-divergent) walk.
  extern __shared__ float lds[];
  float* tcA = lds; float* wA = tcA + (size_t)S * RPB; float* cdfA = wA + (size_t)S * RPB; float* zfA = cdfA + (size_t)S * RPB;
  float* mgA = zfA + (size_t)F * RPB;
  constexpr int L = 64 / RPB;
  const int lane = threadIdx.x, q = lane & (L - 1), rl = lane / L;     // rl = ray within the block
  const int r0 = blockIdx.x * RPB + rl;
  const int r = r0 < B ? r0 : B - 1;
  const int nb = S - 1;        // number of bin edges / cdf entries
  const int nw = S - 2;        // number of weights
  for (int i = q; i < S; i += L) {
    tcA[i * RPB + rl] = path_pd[(size_t)jitter[i] * B + r].w;
    wA[i * RPB + rl] = weights[(size_t)i * B + r];
  }
  __syncthreads();
  auto acc4 = [&](float a, float p) -> float {      // (((a + p0) + p1) + p2) + ...
#pragma unroll
    for (int i = 0; i < L; ++i) a = fadd(a, ray_bcast<L>(p, i));
    return a;
  };
  // weight_sum, padding (model_utils.py:327-331): sequential sum of w[1..S-2]
  float wsum = 0.f;
  for (int j = 0; j < nw; j += L) {
    const int i = j + q;
    wsum = acc4(wsum, i < nw ? wA[(i + 1) * RPB + rl] : 0.f);
  }
  const float padding = fmaxf(0.f, fsub(1e-5f, wsum));
  const float padw = fdiv(padding, (float)nw);
  wsum = fadd(wsum, padding);
  // cdf[0] = 0, cdf[k] = min(1, P_{k-1}) for 1 <= k <= nb-2 with P_m = P_{m-1} + (w[m+1] + padw) / wsum, cdf[nb-1] = 1  (:335-340)
  float cum = 0.f;
  for (int j = 0; j < nw; j += L) {
    const int m = j + q;
    const float term = m < nw ? fdiv(fadd(wA[(m + 1) * RPB + rl], padw), wsum) : 0.f;
    // the serial code starts the running sum AT the first term (no 0 + term), so P_0 is the term itself
    float mine = 0.f;
#pragma unroll
    for (int i = 0; i < L; ++i) {
      const float ti = ray_bcast<L>(term, i);
      cum = (j == 0 && i == 0) ? ti : fadd(cum, ti);
      if (q == i) mine = cum;
    }
    if (m + 1 <= nb - 2) cdfA[(m + 1) * RPB + rl] = fminf(1.f, mine);
  }
  if (q == 0) { cdfA[rl] = 0.f; cdfA[(nb - 1) * RPB + rl] = 1.f; }
  __syncthreads();
  // fine depths: interval i = #{k in [1, nb-2] : cdf[k] <= u} (the walk of :360-370), then the affine map inside it (:372-373)
  for (int j = q; j < F; j += L) {
    const float uj = u_per_ray ? u[(size_t)j * B + r] : u[j];
    int lo = 1, hi = nb - 1;                                       // first k in [1, nb-1) with cdf[k] > uj
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (cdfA[mid * RPB + rl] > uj) hi = mid; else lo = mid + 1; }
    const int i = lo - 1;
    const float c0 = cdfA[i * RPB + rl], c1 = cdfA[(i + 1) * RPB + rl];
    const float ta = tcA[i * RPB + rl], tb = tcA[(i + 1) * RPB + rl], tcx = tcA[(i + 2) * RPB + rl];
    const float b0 = fmul(0.5f, fadd(tb, ta)), b1 = fmul(0.5f, fadd(tcx, tb));     // mids (models.py:371)
    float t = fdiv(fsub(uj, c0), fsub(c1, c0));
    if (t != t) t = 0.f;                              // nan_to_num(., 0): NaN -> 0, inf -> +-FLT_MAX then clip
    t = fminf(fmaxf(t, 0.f), 1.f);
    zfA[j * RPB + rl] = fadd(b0, fmul(t, fsub(b1, b0)));
  }
  __syncthreads();
  // merge of the two sorted lists (jnp.sort of the concatenation, :405; coarse first on ties): rank by binary search
  for (int i = q; i < S; i += L) {
    const float z = tcA[i * RPB + rl];
    int lo = 0, hi = F;                                            // #{j : zf[j] < z}
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (zfA[mid * RPB + rl] < z) lo = mid + 1; else hi = mid; }
    mgA[(i + lo) * RPB + rl] = z;
  }
  for (int j = q; j < F; j += L) {
    const float z = zfA[j * RPB + rl];
    int lo = 0, hi = S;                                            // #{i : tc[i] <= z}
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (tcA[mid * RPB + rl] <= z) lo = mid + 1; else hi = mid; }
    mgA[(j + lo) * RPB + rl] = z;
  }
  __syncthreads();
  // coalesced write-out: RPB consecutive rays per segment
  const int total = S + F;
  const int rr = lane % RPB;
  if (blockIdx.x * RPB + rr < B)
    for (int p = lane / RPB; p < total; p += 64 / RPB) zbuf[(size_t)p * B + blockIdx.x * RPB + rr] = mgA[p * RPB + rr];
}

__global__ void __launch_bounds__(256) resample_gather_kernel(const float4* __restrict__ path_pd, const float4* __restrict__ path_dr,
                                                              int N, int B, const float* __restrict__ zbuf, long long total,
                                                              float4* __restrict__ rows_pd, float4* __restrict__ rows_dr,
                                                              int* __restrict__ node_idx) {
  const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= total) return;
  const int r = (int)(o % B);
  const float z = zbuf[o];
  auto D = [&](int k) -> float { return path_pd[(size_t)k * B + r].w; };
  const float d0 = D(0), dl = D(N - 1);
  const float inv_step = (float)(N - 1) / fmaxf(dl - d0, 1e-30f);
  float gf = (z - d0) * inv_step + 1.0f;
  gf = fminf(fmaxf(gf, 0.f), (float)N);
  const int c = (int)gf;
  // p = #(node depth < z) = smallest p in [0, N] with p == N or D(p) >= z
  int lo = 0, hi = N;
  if (c < N && D(c) < z) {
    lo = c + 1;
    int st = 1;
    while (lo < N) {
      const int t = lo + st - 1 < N - 1 ? lo + st - 1 : N - 1;
      if (D(t) < z) { lo = t + 1; st <<= 1; } else { hi = t; break; }
    }
  } else {
    hi = c;
    int st = 1;
    while (hi > 0) {
      const int t = hi - st > 0 ? hi - st : 0;
      if (D(t) >= z) { hi = t; st <<= 1; } else { lo = t + 1; break; }
    }
    if (hi == 0) lo = 0;
  }
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (D(mid) < z) lo = mid + 1; else hi = mid;
  }
  const int idx = lo > 0 ? lo - 1 : 0;                  // y = hstack([y[0], y, y[-1]])[j] -> max(j-1, 0)
  const float4 pd = path_pd[(size_t)idx * B + r];
  const float4 dr = path_dr[(size_t)idx * B + r];
  const float dz = fsub(z, pd.w);
  rows_pd[o] = make_float4(fadd(pd.x, fmul(dr.x, dz)), fadd(pd.y, fmul(dr.y, dz)), fadd(pd.z, fmul(dr.z, dz)), z);
  rows_dr[o] = dr;
  if (node_idx) node_idx[o] = idx;
}

}  // namespace rnerf

using namespace rnerf;

// lanes per ray of the compositing kernels (they are bound by the latency of a ray's chain of sample groups, not by throughput): 64 while a
// ray per wave still fits one wave per SIMD (<= 1024 rays), 16 up to 8192 rays, 4 beyond.  Measured, forward / backward in us incl. launch
// (round 4): 128 or 512 rays x 192 samples 41 / 69 (4 lanes), 19 / 26 (16), 20 / 14-17 (64); 4096 x 128: 28 / 48, 20 / 22,
// 63 / 81; 4096 x 192: 48 / 72, 27 / 32, 85 / 112; 32768 x 128: 53 / 85, 92 / 140, 364 / 444.  RNERF_COMPOSITE_LANES=4|16|64 forces one (A/B, tests).
static int composite_lanes(int32_t B) {
  static const int forced = [] { const char* e = RNERF_ENV("RNERF_COMPOSITE_LANES"); const int v = e ? atoi(e) : 0; return (v == 4 || v == 16 || v == 64) ? v : 0; }();
  if (forced) return forced;
  return B <= 1024 ? 64 : (B <= 8192 ? 16 : 4);
}

extern "C" int rnerf_composite(const float* raw, const float* rows_pd, const float* rows_dr,
                               const int32_t* node_of_sample, int32_t S, int32_t B, const float* bkgd, int white_bkgd,
                               double rgb_padding, double sigma_bias, float* rgb, float* dist, float* acc, float* trans,
                               float* trans_bkgd, float* weights, float* alpha, int mask_mode, const double* bbox, void* stream) {
  RNERF_CHECK_ARG(raw && rows_pd && rows_dr && rgb && dist && acc && trans && trans_bkgd, "rnerf_composite: null pointer");
  RNERF_CHECK_ARG(mask_mode >= 0 && mask_mode <= 3 && (mask_mode == 0 || bbox), "rnerf_composite: mask_mode 1 / 2 / 3 needs a bbox");
  float bb[6] = {0, 0, 0, 0, 0, 0};
  if (mask_mode != 0) for (int i = 0; i < 6; ++i) bb[i] = (float)bbox[i];
  RNERF_CHECK_ARG(S >= 1 && B >= 1, "rnerf_composite: need S >= 1 and B >= 1");
  RNERF_CHECK_ARG((((uintptr_t)raw | (uintptr_t)rows_pd | (uintptr_t)rows_dr) & 15) == 0, "rnerf_composite: float4 buffers must be 16-byte aligned");
#define RNERF_COMPOSITE_LAUNCH(LL)                                                                                              \
  hipLaunchKernelGGL(composite_kernel<LL>, dim3((unsigned)(((long long)B * LL + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const float4*)raw, \
                     (const float4*)rows_pd, (const float4*)rows_dr, node_of_sample, S, B, bkgd, white_bkgd,                     \
                     (float)(1 + 2 * rgb_padding), (float)rgb_padding, (float)sigma_bias, rgb, dist, acc, trans, trans_bkgd,     \
                     weights, alpha, mask_mode, bb[0], bb[1], bb[2], bb[3], bb[4], bb[5])
  const int lanes = composite_lanes(B);
  if (lanes == 4) RNERF_COMPOSITE_LAUNCH(4); else if (lanes == 16) RNERF_COMPOSITE_LAUNCH(16); else RNERF_COMPOSITE_LAUNCH(64);
#undef RNERF_COMPOSITE_LAUNCH
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_resample(const float* path_pd, const float* path_dr, int32_t num_nodes, int32_t B,
                              const int32_t* jitter, int32_t S, const float* weights, const float* u, int32_t u_per_ray,
                              int32_t num_fine, float* rows_pd, float* rows_dr, int32_t* node_idx, float* scratch,
                              void* stream) {
  RNERF_CHECK_ARG(path_pd && path_dr && jitter && weights && rows_pd && rows_dr && scratch, "rnerf_resample: null pointer");
  RNERF_CHECK_ARG(u || num_fine == 0, "rnerf_resample: u must be given (use linspace(0,1-eps,F) for randomized=False)");
  RNERF_CHECK_ARG(S >= 3 && B >= 1 && num_nodes >= 2 && num_fine >= 0, "rnerf_resample: need S >= 3, B >= 1, num_nodes >= 2");
  const long long need = 4 * (long long)S + 2 * (long long)num_fine;      // floats of LDS staging per ray
  RNERF_CHECK_ARG(need <= 40960, "rnerf_resample: 4*S + 2*num_fine > 40960 does not fit the 160 KiB LDS staging even at one ray per block");
  RNERF_CHECK_ARG((((uintptr_t)path_pd | (uintptr_t)path_dr | (uintptr_t)rows_pd | (uintptr_t)rows_dr) & 15) == 0,
                  "rnerf_resample: float4 buffers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  // rays per block: 64 / (lanes per ray), the lanes as for the compositing kernels (few rays: more lanes each), and no more rays than the
  // 160 KiB of LDS hold
  int rpb = 64 / composite_lanes(B);
  if (rpb > 4 && need > 2560) rpb = 4;
  if (rpb > 1 && need > 10240) rpb = 1;
  const size_t lds = (size_t)need * rpb * sizeof(float);
  static DeviceOnce attr_set;
  if (attr_set.need()) {
    RNERF_CHECK_HIP(hipFuncSetAttribute((const void*)resample_depths_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
    RNERF_CHECK_HIP(hipFuncSetAttribute((const void*)resample_depths_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
    RNERF_CHECK_HIP(hipFuncSetAttribute((const void*)resample_depths_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
    attr_set.set();
  }
  const dim3 rgrid((unsigned)((B + rpb - 1) / rpb));
  if (rpb == 16)
    hipLaunchKernelGGL(resample_depths_kernel<16>, rgrid, dim3(64), lds, st, (const float4*)path_pd, B, jitter, S, weights, u, u_per_ray, num_fine, scratch);
  else if (rpb == 4)
    hipLaunchKernelGGL(resample_depths_kernel<4>, rgrid, dim3(64), lds, st, (const float4*)path_pd, B, jitter, S, weights, u, u_per_ray, num_fine, scratch);
  else
    hipLaunchKernelGGL(resample_depths_kernel<1>, rgrid, dim3(64), lds, st, (const float4*)path_pd, B, jitter, S, weights, u, u_per_ray, num_fine, scratch);
  const long long total = (long long)(S + num_fine) * B;
  hipLaunchKernelGGL(resample_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float4*)path_pd,
                     (const float4*)path_dr, num_nodes, B, scratch, total, (float4*)rows_pd, (float4*)rows_dr, node_idx);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

// The stratified draws of sorted_piecewise_constant_pdf (rnerf/model_utils.py:345-354) on the device:
// u[b][f] = min(f*s + uniform(key, [B,F], maxval = s - eps)[b][f], 1 - eps), written sample-major float[F][B].
// jax.random.uniform -> threefry2x32-20 over the counters 0..B*F-1 split in two halves (x0 = first half, x1 = second half).
__device__ __forceinline__ unsigned rotl32(unsigned x, int r) { return (x << r) | (x >> (32 - r)); }
__global__ void __launch_bounds__(256) stratified_u_kernel(unsigned k0, unsigned k1, int B, int F, float s, float maxval, float one_m_eps,
                                                           float* __restrict__ u) {
  const long long size = (long long)B * F, half = (size + 1) / 2;
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= half) return;
  const unsigned ks[3] = {k0, k1, k0 ^ k1 ^ 0x1BD11BDAu};
  unsigned x0 = (unsigned)j + ks[0];
  unsigned x1 = (j + half < size ? (unsigned)(j + half) : 0u) + ks[1];
  const int rot[2][4] = {{13, 15, 26, 6}, {17, 29, 16, 24}};
#pragma unroll
  for (int i = 0; i < 5; ++i) {
#pragma unroll
    for (int q = 0; q < 4; ++q) { x0 += x1; x1 = rotl32(x1, rot[i & 1][q]); x1 ^= x0; }
    x0 += ks[(i + 1) % 3];
    x1 += ks[(i + 2) % 3] + (unsigned)(i + 1);
  }
  auto put = [&](long long e, unsigned bits) {
    const int b = (int)(e / F), f = (int)(e % F);
    const float fl = fsub(__uint_as_float((bits >> 9) | 0x3F800000u), 1.0f);
    const float r = fmaxf(0.0f, fadd(fmul(fl, maxval), 0.0f));
    u[(size_t)f * B + b] = fminf(fadd(fmul((float)f, s), r), one_m_eps);
  };
  put(j, x0);
  if (j + half < size) put(j + half, x1);
}

extern "C" int rnerf_stratified_u(const uint32_t* key, int32_t B, int32_t num_fine, float* u, void* stream) {
  RNERF_CHECK_ARG(key && u, "rnerf_stratified_u: null pointer");
  RNERF_CHECK_ARG(B >= 1 && num_fine >= 1, "rnerf_stratified_u: need B >= 1 and num_fine >= 1");
  const double eps = 1.1920928955078125e-07;
  const double s = 1.0 / num_fine;
  const long long half = ((long long)B * num_fine + 1) / 2;
  hipLaunchKernelGGL(stratified_u_kernel, dim3((unsigned)((half + 255) / 256)), dim3(256), 0, (hipStream_t)stream, key[0], key[1], B, num_fine,
                     (float)s, (float)(s - eps), (float)(1.0 - eps), u);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

// Pinhole ray generation for rows [row0, row0 + rows) of one H x W view (rnerf/datasets.py:216-242 Blender, :486-518 OpenCV), in
// the reference's fp32 op order: one thread per pixel, no host->device ray traffic for full-frame evaluation.
struct RayCam { float r[9]; float t[3]; float fx, fy, cx, cy, pc; int opencv; };
__global__ void __launch_bounds__(256) generate_rays_kernel(RayCam c, int W, int row0, long long n, float* __restrict__ origins,
                                                            float* __restrict__ directions, float* __restrict__ viewdirs) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int col = (int)(i % W), row = row0 + (int)(i / W);
  float cam[3];
  if (!c.opencv) {        // x = arange(w) + pc; ((x - w/2) / focal, -(y - h/2) / focal, -1)        (cx, cy hold w/2, h/2)
    cam[0] = fdiv(fsub(fadd((float)col, c.pc), c.cx), c.fx);
    cam[1] = -fdiv(fsub(fadd((float)row, c.pc), c.cy), c.fy);
    cam[2] = -1.0f;
  } else {                // ((x - cx + pc) / fx, (y - cy + pc) / fy, 1)
    cam[0] = fdiv(fadd(fsub((float)col, c.cx), c.pc), c.fx);
    cam[1] = fdiv(fadd(fsub((float)row, c.cy), c.pc), c.fy);
    cam[2] = 1.0f;
  }
  float d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = fadd(fadd(fmul(cam[0], c.r[3 * k]), fmul(cam[1], c.r[3 * k + 1])), fmul(cam[2], c.r[3 * k + 2]));
  const float nrm = fsqrt(fadd(fadd(fmul(d[0], d[0]), fmul(d[1], d[1])), fmul(d[2], d[2])));
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    origins[3 * i + k] = c.t[k];
    if (directions) directions[3 * i + k] = d[k];
    viewdirs[3 * i + k] = fdiv(d[k], nrm);
  }
}

// ---- the gather half of Dataset._next_train (rnerf/datasets.py:151-176,178-197) on the device.  The reference keeps the rays
// of every training view as host arrays ([n_img, H*W, 3] x 3) and indexes them and the images with the drawn ray indices; here the images
// and the cameras are resident on the device, a batch is "B flat indices (image * H * W + row * W + column)", and the rays of exactly those
// pixels are generated on the fly with the arithmetic of generate_rays_kernel — the same bits as indexing the reference's arrays — next
// to the pixel gather: one thread per ray, no ray arrays in memory, no per-step host tensor work.
__device__ __forceinline__ void pinhole_ray(const float* __restrict__ r, float fx, float fy, float cx, float cy, float pc, int opencv, int col, int row,
                                            float (&d)[3], float (&v)[3]) {
  float cam[3];
  if (!opencv) {
    cam[0] = fdiv(fsub(fadd((float)col, pc), cx), fx);
    cam[1] = -fdiv(fsub(fadd((float)row, pc), cy), fy);
    cam[2] = -1.0f;
  } else {
    cam[0] = fdiv(fadd(fsub((float)col, cx), pc), fx);
    cam[1] = fdiv(fadd(fsub((float)row, cy), pc), fy);
    cam[2] = 1.0f;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = fadd(fadd(fmul(cam[0], r[3 * k]), fmul(cam[1], r[3 * k + 1])), fmul(cam[2], r[3 * k + 2]));
  const float nrm = fsqrt(fadd(fadd(fmul(d[0], d[0]), fmul(d[1], d[1])), fmul(d[2], d[2])));
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = fdiv(d[k], nrm);
}
struct BatchCam { float fx, fy, cx, cy, pc; int opencv; };
__global__ void __launch_bounds__(256) sample_batch_kernel(const float* __restrict__ camtoworlds, BatchCam c, int W, int H, int n_img,
                                                           const float* __restrict__ images, int channels, const long long* __restrict__ idx,
                                                           int B, float* __restrict__ origins, float* __restrict__ directions,
                                                           float* __restrict__ viewdirs, float* __restrict__ pixels, int* __restrict__ bad) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  long long i = idx[b];
  const long long hw = (long long)H * W;
  if (i < 0 || i >= hw * n_img) { atomicAdd(bad, 1); i = 0; }      // reported by the host wrapper: never read out of bounds
  const int img = (int)(i / hw), pix = (int)(i - (long long)img * hw);
  const int row = pix / W, col = pix - row * W;
  const float* __restrict__ m = camtoworlds + 12 * img;             // [3][4] row-major: rotation | translation
  const float r[9] = {m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]};
  float d[3], v[3];
  pinhole_ray(r, c.fx, c.fy, c.cx, c.cy, c.pc, c.opencv, col, row, d, v);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    origins[3 * b + k] = m[4 * k + 3];
    if (directions) directions[3 * b + k] = d[k];
    viewdirs[3 * b + k] = v[k];
  }
  if (pixels) {
    const float* __restrict__ src = images + (size_t)i * channels;
    for (int k = 0; k < channels; ++k) pixels[(size_t)b * channels + k] = src[k];
  }
}

// ---- mip-style integrated positional encoding along the CURVED ray (rnerf/mip.py:26-57,60-91,116-175), as the commented
// call sites would use it (rnerf/models.py:249-254): the coarse samples of a marched path are the axes of conical frusta between
// consecutive depths; each frustum becomes a diagonal Gaussian whose mean is accumulated ALONG the bent path (cumsum of d * dt), and the
// encoding is exp(-var / 2) * sin(.) of the scaled mean.  One lane per ray (the cumulative mean is a serial sum per ray, in sample
// order like the oracle); rows are sample-major, so every load and store of a wave is contiguous.
__device__ __forceinline__ float safe_sin_f(float x) {      // math_utils.safe_sin: sin(where(|x| < 100 pi, x, x % (100 pi)))
  const float t = 314.159271f;                              // f32(100 pi)
  return sinf(fabsf(x) < t ? x : x - floorf(x / t) * t);
}
__global__ void __launch_bounds__(64) ipe_kernel(const float4* __restrict__ rows_pd, const float4* __restrict__ rows_dr,
                                                 const int* __restrict__ node_of_sample, int S, int B, const float* __restrict__ radii,
                                                 float near, int min_deg, int max_deg, float4* __restrict__ out_mean,
                                                 float4* __restrict__ out_cov, float* __restrict__ enc) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float br = radii[b];
  const int L = max_deg - min_deg;
  auto rec = [&](int s) -> size_t { return (size_t)(node_of_sample ? node_of_sample[s] : s) * B + b; };
  const float4 p0 = rows_pd[rec(0)];
  float run[3] = {0.f, 0.f, 0.f};
  float t_prev_mean = near;                                  // t = [t_mean_0 - near, t_mean_s - t_mean_(s-1)]  (mip.py:38)
  float t0 = p0.w;
  for (int s = 0; s < S; ++s) {
    const float4 dr = rows_dr[rec(s)];
    const float t1 = s + 1 < S ? rows_pd[rec(s + 1)].w : fadd(t0, 1e-3f);      // t_vals = [dist_c, last + 1e-3]
    const float mu = fdiv(fadd(t0, t1), 2.f), hw = fdiv(fsub(t1, t0), 2.f);
    const float mu2 = fmul(mu, mu), hw2 = fmul(hw, hw), hw4 = fmul(hw2, hw2);
    const float den = fadd(fmul(3.f, mu2), hw2);
    const float t_mean = fadd(mu, fdiv(fmul(fmul(2.f, mu), hw2), den));
    const float t_var = fsub(fdiv(hw2, 3.f), fmul((float)(4.0 / 15.0), fdiv(fmul(hw4, fsub(fmul(12.f, mu2), hw2)), fmul(den, den))));
    const float r_var = fmul(fmul(br, br), fsub(fadd(fdiv(mu2, 4.f), fmul((float)(5.0 / 12.0), hw2)), fdiv(fmul((float)(4.0 / 15.0), hw4), den)));
    const float t = fsub(t_mean, t_prev_mean);
    t_prev_mean = t_mean;
    const float d[3] = {dr.x, dr.y, dr.z};
    const float mag = fmaxf(1e-10f, fadd(fadd(fmul(d[0], d[0]), fmul(d[1], d[1])), fmul(d[2], d[2])));
    float mean[3], cov[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      run[c] = fadd(run[c], fmul(d[c], t));
      const float dd = fmul(d[c], d[c]);
      mean[c] = fadd(run[c], c == 0 ? p0.x : (c == 1 ? p0.y : p0.z));            // + origins[:, 0:1]: the first coarse sample's position
      cov[c] = fadd(fmul(t_var, dd), fmul(r_var, fsub(1.f, fdiv(dd, mag))));
    }
    const size_t o = (size_t)s * B + b;
    if (out_mean) out_mean[o] = make_float4(mean[0], mean[1], mean[2], t_mean);
    if (out_cov) out_cov[o] = make_float4(cov[0], cov[1], cov[2], t_var);
    if (enc) {
      float* e = enc + o * (size_t)(6 * L);
      for (int k = 0; k < L; ++k) {
        const float sc = (float)(1 << (min_deg + k));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float y = fmul(mean[c], sc), yv = fmul(cov[c], fmul(sc, sc));
          const float w = expf(fmul(-0.5f, yv));
          e[3 * k + c] = fmul(w, safe_sin_f(y));
          e[3 * L + 3 * k + c] = fmul(w, safe_sin_f(fadd(y, 1.5707963705062866f)));
        }
      }
    }
    t0 = t1;
  }
}

extern "C" int rnerf_integrated_pos_enc(const float* rows_pd, const float* rows_dr, const int32_t* node_of_sample, int32_t S, int32_t B,
                                        const float* radii, double near, int32_t min_deg, int32_t max_deg, float* out_mean4, float* out_cov4,
                                        float* out_enc, void* stream) {
  RNERF_CHECK_ARG(rows_pd && rows_dr && radii && (out_mean4 || out_cov4 || out_enc), "rnerf_integrated_pos_enc: null pointer");
  RNERF_CHECK_ARG(S >= 1 && B >= 1 && min_deg >= 0 && max_deg > min_deg && max_deg <= 30, "rnerf_integrated_pos_enc: need S, B >= 1 and 0 <= min_deg < max_deg <= 30");
  RNERF_CHECK_ARG((((uintptr_t)rows_pd | (uintptr_t)rows_dr | (uintptr_t)out_mean4 | (uintptr_t)out_cov4) & 15) == 0, "rnerf_integrated_pos_enc: float4 buffers must be 16-byte aligned");
  hipLaunchKernelGGL(ipe_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const float4*)rows_pd, (const float4*)rows_dr, node_of_sample, S, B,
                     radii, (float)near, min_deg, max_deg, (float4*)out_mean4, (float4*)out_cov4, out_enc);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_generate_rays(const float* camtoworld, int32_t opencv, double fx, double fy, double cx, double cy, double pixel_center,
                                   int32_t W, int32_t row0, int32_t rows, float* origins, float* directions, float* viewdirs, void* stream) {
  RNERF_CHECK_ARG(camtoworld && origins && viewdirs, "rnerf_generate_rays: null pointer");
  RNERF_CHECK_ARG(W >= 1 && rows >= 1 && row0 >= 0, "rnerf_generate_rays: need W >= 1, rows >= 1, row0 >= 0");
  RayCam c;
  for (int k = 0; k < 3; ++k) { for (int j = 0; j < 3; ++j) c.r[3 * k + j] = camtoworld[4 * k + j]; c.t[k] = camtoworld[4 * k + 3]; }
  c.fx = (float)fx; c.fy = (float)fy; c.cx = (float)cx; c.cy = (float)cy; c.pc = (float)pixel_center; c.opencv = opencv;
  const long long n = (long long)rows * W;
  hipLaunchKernelGGL(generate_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, c, W, row0, n, origins, directions,
                     viewdirs);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_sample_batch(const float* camtoworlds, int32_t n_img, int32_t opencv, double fx, double fy, double cx, double cy, double pixel_center,
                                  int32_t W, int32_t H, const float* images, int32_t channels, const int64_t* ray_indices, int32_t B, float* origins,
                                  float* directions, float* viewdirs, float* pixels, int32_t* bad_count, void* stream) {
  RNERF_CHECK_ARG(camtoworlds && ray_indices && origins && viewdirs && bad_count, "rnerf_sample_batch: null pointer");
  RNERF_CHECK_ARG((images == nullptr) == (pixels == nullptr), "rnerf_sample_batch: give both images and pixels (a training batch) or neither (rays only: the env-map patch)");
  RNERF_CHECK_ARG(n_img >= 1 && W >= 1 && H >= 1 && B >= 1, "rnerf_sample_batch: need n_img, W, H, B >= 1");
  RNERF_CHECK_ARG(images == nullptr || (channels >= 1 && channels <= 4), "rnerf_sample_batch: 1..4 channels");
  BatchCam c;
  c.fx = (float)fx; c.fy = (float)fy; c.cx = (float)cx; c.cy = (float)cy; c.pc = (float)pixel_center; c.opencv = opencv;
  hipLaunchKernelGGL(sample_batch_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, camtoworlds, c, W, H, n_img, images,
                     channels, (const long long*)ray_indices, B, origins, directions, viewdirs, pixels, bad_count);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_loss_reduce(const float* rgb_c, const float* rgb_f, const float* trans_f, const float* trans_bkgd_f,
                                 const float* pixels, int32_t B, float* sums, void* stream) {
  RNERF_CHECK_ARG(rgb_f && trans_f && trans_bkgd_f && pixels && sums, "rnerf_loss_reduce: null pointer");
  RNERF_CHECK_ARG(B >= 1, "rnerf_loss_reduce: B must be >= 1");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(1024), 0, st, rgb_c, rgb_f, trans_f, trans_bkgd_f, pixels, B, sums);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

// ---- the scalar tail of loss_fn in two small kernels (instead of ~35 framework elementwise launches per step) ----------------
// env-map smoothness (train.py:127-130): loss = mean(0.5 dv^2 + 0.5 dh^2) over the [ps-1, ps, 3] / [ps, ps-1, 3] differences of the
// patch; d_out = scale * d loss / d rgb_env; the un-normalised sum of squares of block b goes to loss_sum[4 + b] — one partial per block,
// summed in index order by train_stats_kernel: no float atomics, the same bits from run to run (and nothing to zero beforehand).
__global__ void __launch_bounds__(256) env_smooth_kernel(const float* __restrict__ x, int ps, float k, float* __restrict__ d_out,
                                                         float* __restrict__ loss_sum) {
  __shared__ float wsum[4];
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = ps * ps * 3;
  float part = 0.f;
  if (id < n) {
    const int c = id % 3, j = (id / 3) % ps, i = id / (3 * ps);
    const float v = x[id];
    float g = 0.f;
    if (i > 0) g += v - x[id - 3 * ps];
    if (i < ps - 1) { const float d = x[id + 3 * ps] - v; g -= d; part += 0.5f * d * d; }
    if (j > 0) g += v - x[id - 3];
    if (j < ps - 1) { const float d = x[id + 3] - v; g -= d; part += 0.5f * d * d; }
    d_out[id] = g * k;
    (void)c;
  }
  for (int o = 32; o > 0; o >>= 1) part += __shfl_down(part, o);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) loss_sum[4 + blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// sum x^2 by ONE workgroup in a fixed order (per-thread strided partial sums, then a fixed tree): *out = the sum — assigned, not
// accumulated; no float atomics, the same bits from run to run.  5 MB of parameters take ~40 us on one CU: in the training step it runs
// on the aux stream beside the coarse forward (csrc/pipeline.hip), off the critical path.
__global__ void __launch_bounds__(1024) sumsq_kernel(const float* __restrict__ x, long long n, float* __restrict__ out) {
  __shared__ float wsum[16];
  const int tid = threadIdx.x;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  const long long n4 = ((uintptr_t)x & 15) == 0 ? n / 4 : 0;               // float4 body (unaligned buffers: scalar loop only)
  const float4* __restrict__ x4 = (const float4*)x;
  // four independent 16-byte loads in flight per thread (one CU pulls ~64 B per clock at best: 5 MB in ~40 us; with one load per iteration
  // the loop ran at a latency-bound 94 us, on the critical path of the staged step — VERDICT r05 weak #6).  Same partial sums per thread
  // (s0..s3 take the same elements in the same order): the same bits as before.
  long long i = tid;
  for (; i + 3 * 1024 < n4; i += 4 * 1024) {
    const float4 v0 = x4[i], v1 = x4[i + 1024], v2 = x4[i + 2048], v3 = x4[i + 3072];
    s0 += v0.x * v0.x; s1 += v0.y * v0.y; s2 += v0.z * v0.z; s3 += v0.w * v0.w;
    s0 += v1.x * v1.x; s1 += v1.y * v1.y; s2 += v1.z * v1.z; s3 += v1.w * v1.w;
    s0 += v2.x * v2.x; s1 += v2.y * v2.y; s2 += v2.z * v2.z; s3 += v2.w * v2.w;
    s0 += v3.x * v3.x; s1 += v3.y * v3.y; s2 += v3.z * v3.z; s3 += v3.w * v3.w;
  }
  for (; i < n4; i += 1024) { const float4 v = x4[i]; s0 += v.x * v.x; s1 += v.y * v.y; s2 += v.z * v.z; s3 += v.w * v.w; }
  for (long long i = 4 * n4 + tid; i < n; i += 1024) s0 += x[i] * x[i];
  float s = (s0 + s1) + (s2 + s3);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  if ((tid & 63) == 0) wsum[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int w = 0; w < 16; ++w) t += wsum[w];
    *out = t;
  }
}

// st[0] loss, st[1] loss_c, st[2] loss_bg, st[3] loss_bg_smooth, st[4] weight_l2, st[6] psnr, st[7] psnr_c (utils.Stats, train.py:147-162)
__global__ void train_stats_kernel(const float* __restrict__ sums, float inv3B, int two_levels, float bg_on, const float* __restrict__ env_sum,
                                   int env_blocks, float env_scale, float frozen_sq, float inv_n_all, float* __restrict__ st) {
  // the env-map term's per-block partials (env_smooth_kernel), summed in index order: lane l takes partials l, l + 64, ..., then a fixed tree
  float env = 0.f;
  if (env_sum) {
    for (int b = threadIdx.x; b < env_blocks; b += 64) env += env_sum[4 + b];
    for (int o = 32; o > 0; o >>= 1) env += __shfl_down(env, o);
  }
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float kp = -4.342944819032518f;                 // -10 / ln 10 (utils.compute_psnr)
  const float loss = sums[0] * inv3B;
  st[0] = loss;
  st[6] = kp * logf(loss);
  if (two_levels) { const float lc = sums[1] * inv3B; st[1] = lc; st[7] = kp * logf(lc); }
  st[2] = bg_on * sums[2] / (sums[3] + 1.0f);
  if (env_sum) st[3] = env * env_scale;
  st[4] = (st[5] + frozen_sq) * inv_n_all;              // st[5]: sum of squares of the trained parameters (sumsq_kernel)
  st[5] = 0.f;
}

extern "C" size_t rnerf_env_smooth_sum_floats(int32_t ps) { return ps >= 2 ? 4 + (size_t)((ps * ps * 3 + 255) / 256) : 4; }

extern "C" int rnerf_env_smooth_backward(const float* rgb_env, int32_t ps, double grad_scale, float* d_out, float* loss_sum, void* stream) {
  RNERF_CHECK_ARG(rgb_env && d_out && loss_sum && ps >= 2, "rnerf_env_smooth_backward: null pointer or ps < 2");
  hipStream_t st = (hipStream_t)stream;
  const int n = ps * ps * 3;
  const double m = (double)(ps - 1) * ps * 3;
  hipLaunchKernelGGL(env_smooth_kernel, dim3((n + 255) / 256), dim3(256), 0, st, rgb_env, ps, (float)(grad_scale / m), d_out, loss_sum);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_train_stats(const float* sums, int32_t B, int32_t two_levels, double bg_scale, const float* env_loss_sum, int32_t ps,
                                 double env_on, const float* theta, int64_t n_theta, double frozen_sq, int64_t n_all, float* stats8,
                                 void* stream) {
  RNERF_CHECK_ARG(sums && stats8 && B >= 1 && n_theta >= 1 && n_all >= n_theta, "rnerf_train_stats: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (theta) hipLaunchKernelGGL(sumsq_kernel, dim3(1), dim3(1024), 0, st, theta, (long long)n_theta, stats8 + 5);      // NULL: rnerf_theta_sumsq ran already
  const double m = ps >= 2 ? (double)(ps - 1) * ps * 3 : 1.0;
  hipLaunchKernelGGL(train_stats_kernel, dim3(1), dim3(64), 0, st, sums, (float)(1.0 / (3.0 * B)), two_levels, (float)bg_scale, env_loss_sum,
                     ps >= 2 ? (ps * ps * 3 + 255) / 256 : 0, (float)(env_on / m), (float)frozen_sq, (float)(1.0 / (double)n_all), stats8);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_theta_sumsq(const float* theta, int64_t n_theta, float* stats8, void* stream) {
  RNERF_CHECK_ARG(theta && stats8 && n_theta >= 1, "rnerf_theta_sumsq: bad arguments");
  hipLaunchKernelGGL(sumsq_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, theta, (long long)n_theta, stats8 + 5);
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}

extern "C" int rnerf_composite_backward(const float* raw, const float* rows_pd, const float* rows_dr, const int32_t* node_of_sample,
                                        int32_t S, int32_t B, const float* bkgd, double rgb_padding, double sigma_bias,
                                        const float* rgb, const float* pixels, const float* trans, const float* trans_bkgd,
                                        const float* sums, double mse_scale, double bg_scale, float* d_raw, float* d_bkgd,
                                        int accumulate_bkgd, int white_bkgd, int mask_mode, const double* bbox, void* stream) {
  RNERF_CHECK_ARG((mask_mode == 0 || mask_mode == 1 || mask_mode == 3) && (mask_mode == 0 || bbox),
                  "rnerf_composite_backward: mask_mode must be 0, 1 (bd_cut pair) or 3 (use_mask_bbox), the last two with a bbox");
  const double* bd_cut_bbox = mask_mode != 0 ? bbox : nullptr;
  RNERF_CHECK_ARG(raw && rows_pd && rows_dr && bkgd && rgb && pixels && d_raw && d_bkgd, "rnerf_composite_backward: null pointer");
  RNERF_CHECK_ARG(bg_scale == 0.0 || (trans && trans_bkgd && sums), "rnerf_composite_backward: bg term needs trans, trans_bkgd and sums");
  RNERF_CHECK_ARG(S >= 1 && B >= 1, "rnerf_composite_backward: need S >= 1 and B >= 1");
  RNERF_CHECK_ARG((((uintptr_t)raw | (uintptr_t)rows_pd | (uintptr_t)rows_dr | (uintptr_t)d_raw) & 15) == 0,
                  "rnerf_composite_backward: float4 buffers must be 16-byte aligned");
#define RNERF_COMPOSITE_BWD_LAUNCH(LL)                                                                                          \
  hipLaunchKernelGGL(composite_bwd_kernel<LL>, dim3((unsigned)(((long long)B * LL + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (const float4*)raw, \
                     (const float4*)rows_pd, (const float4*)rows_dr, node_of_sample, S, B, bkgd, (float)(1 + 2 * rgb_padding),   \
                     (float)rgb_padding, (float)sigma_bias, rgb, pixels, trans, trans_bkgd, sums, (float)mse_scale, (float)bg_scale, \
                     (float4*)d_raw, d_bkgd, accumulate_bkgd, mask_mode, bd_cut_bbox ? (float)bd_cut_bbox[0] : 0.f,  \
                     bd_cut_bbox ? (float)bd_cut_bbox[1] : 0.f, bd_cut_bbox ? (float)bd_cut_bbox[2] : 0.f, bd_cut_bbox ? (float)bd_cut_bbox[3] : 0.f, \
                     bd_cut_bbox ? (float)bd_cut_bbox[4] : 0.f, bd_cut_bbox ? (float)bd_cut_bbox[5] : 0.f, white_bkgd)
  const int lanes = composite_lanes(B);
  if (lanes == 4) RNERF_COMPOSITE_BWD_LAUNCH(4); else if (lanes == 16) RNERF_COMPOSITE_BWD_LAUNCH(16); else RNERF_COMPOSITE_BWD_LAUNCH(64);
#undef RNERF_COMPOSITE_BWD_LAUNCH
  RNERF_CHECK_LAUNCH();
  return RNERF_OK;
}
