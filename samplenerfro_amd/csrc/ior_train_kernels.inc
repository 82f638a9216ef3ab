// Training of stage "all*" (SURVEY.md §8f N3): back-propagation through the N-step eikonal recurrence and through so3_mlp.
// Included by mlp.hip inside namespace rnerf.  Reference: rnerf/eikonal_utils.py:29-49,100-124 (the recurrence that
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
// a_p / a_d come from nerfmlp_input_grad_kernel (d loss / d position and direction of every coarse sample: through the position /
// view encodings of Dense_0, the skip concat of Dense_5 and the view layer Dense_10) and from the background MLP's input gradient.

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
