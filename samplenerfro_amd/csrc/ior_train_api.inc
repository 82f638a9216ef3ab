// C ABI of the stage "all*" training pieces (kernels: ior_train_kernels.inc).  Included by mlp.hip after `using namespace rnerf`.

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
  RNERF_CHECK_ARG(grid_fits_u32(gp), "rnerf_march_all_train: grid too large for 32-bit byte offsets (needs a table < 4 GiB)");
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

extern "C" int rnerf_so3_forward_train(const float* so3_params, const float* window10, const float* pts4, int64_t n, void* save, void* stream) {
  RNERF_CHECK_ARG(so3_params && window10 && pts4 && save, "rnerf_so3_forward_train: null pointer");
  RNERF_CHECK_ARG(n >= 1, "rnerf_so3_forward_train: n must be >= 1");
  So3Window w;
  for (int i = 0; i < 10; ++i) w.w[i] = window10[i];
  return launch_so3_16_fwd_train(so3_params, w, pts4, (long long)n, (float*)save, (hipStream_t)stream);      // f16 hi + lo MFMAs (csrc/bkgd16.hip)
}

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
  RNERF_CHECK_ARG(grid_fits_u32(gp), "rnerf_march_adjoint: grid too large for 32-bit byte offsets (needs a table < 4 GiB)");
  const float stepf = (float)((far - near) / (num_nodes - 1));
  hipLaunchKernelGGL(march_adjoint_kernel, dim3((unsigned)((B + 15) / 16)), dim3(64), 0, (hipStream_t)stream, (const float4*)table, gp,
                     (const float4*)path_pd, (const float4*)path_rdn, (const int*)pair_of_node, A12, P12, (const float4*)a_pos, (const float4*)a_dir,
                     (const int*)sample_of_node, B, num_nodes, stepf, (float4*)v4);
  RNERF_CHECK_LAUNCH();
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
