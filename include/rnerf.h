/*
 * rnerf.h — C ABI of librnerf.so, the MI355X (gfx950) implementation of the SampleNeRFRO
 * volumetric-rendering hot path.
 *
 * The reference (alexkeroro86/SampleNeRFRO) has no FFI/plugin layer: the path sits behind
 * Python callables.  Each entry point below names the reference function
 * (file:line under the reference checkout) whose arithmetic it replaces; the Python host
 * (samplenerfro_amd/) re-creates the reference call surface (NerfModel.__call__, render_image,
 * train_step) on top of these.  INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless named h_*;
 *   - nothing is allocated per call; scratch comes from the caller (`*_workspace_bytes`);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *   - return value: 0 = ok, <0 = error (message via rnerf_last_error(), thread local);
 *   - "sample-major" layout: an array indexed [s][b] stores sample/node s of ray b at s*B + b,
 *     so that one-lane-per-ray kernels read and write coalesced.
 *   - a "row record" is two float4 arrays: pd = (pos.x, pos.y, pos.z, dist) and
 *     dr = (dir.x, dir.y, dir.z, 0) with dir already safe-l2-normalised.
 */
#ifndef RNERF_H_
#define RNERF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header: entry points AND struct layouts.  2 (round 5): rnerf_grid carries `layout` (so every later field of rnerf_model
 * moved), rnerf_train_cfg carries grads_stream, rnerf_adam_cfg carries use_lr_override (lr_override alone is ignored).  A
 * consumer compares rnerf_version() with the RNERF_VERSION it was compiled against before the first call (the Python binding does:
 * samplenerfro_amd/_lib.py load()).
 * 3 (round 6): everything that moved after the first version-2 header — rnerf_composite_backward takes `int mask_mode`, rnerf_adam_cfg carries
 * skip_nonfinite, RNERF_ADAM_SCRATCH_FLOATS is 3076 (was 2052), every f16-based packed NerfMLP buffer ends with a bf16x3 range-safe
 * stream (rnerf_nerfmlp_packed_bytes grew) — and this round's additions: enum rnerf_backward gains F16X3_LO8, rnerf_sample_batch.
 * 4: the opt-in schedule fields no caller set are gone.  rnerf_train_cfg ends with aux_stream, grads_stream (nothing in between);
 * rnerf_prefetch ends with side_stream (the march always forks right before the last NerfMLP wgrad); rnerf_bkgd_backward is the only
 * background-MLP backward entry point.  Still 4 with rnerf_flip / rnerf_flip_workspace_bytes, rnerf_visual_hull_*, rnerf_marching_cubes_*,
 * rnerf_mesh_depth, rnerf_mask_dilate, rnerf_vis_*, rnerf_images_prepare, rnerf_errmap_*, rnerf_ssim_summary, rnerf_lpips,
 * rnerf_components_* and rnerf_march_sparse: they are appended, no
 * existing entry point or struct moved (rnerf_prefetch grew by two trailing fields: a caller that fills it by name and zeroes the
 * rest gets the dense march as before). */
#define RNERF_VERSION 4

enum rnerf_status {
  RNERF_OK = 0,
  RNERF_ERR_ARG = -1,   /* bad argument (null pointer, size, alignment) */
  RNERF_ERR_HIP = -2,   /* a HIP runtime call failed */
  RNERF_ERR_UNSUPPORTED = -3
};

/* MLP arithmetic. F32 (rnerf_nerfmlp_pack / rnerf_nerfmlp_forward only) = every Dense as ONE sequential chain of v_fma_f32 per output, then + bias: exact
 * fp32 semantics with a defined summation order — the on-device arbiter of the MFMA precisions (csrc/mlp_f32.hip; ~100 x slower, for
 * parity tests: it separates split-f16 error, the oracle's summation order and real bugs on the device); F16X3 / BF16X3 = hi/lo split of
 * both operands, 3 MFMAs per tile (error ~2^-21 / ~2^-16 per product); F16 / BF16 = single MFMA;
 * F16X2 (forward / inference only) = exact hi+lo f16 weights x activations rounded to f16, 2 MFMAs per tile: the f16x3 operand stream,
 * 2/3 of its matrix work; measured end-to-end |dRGB| vs f16x3 3e-5 .. 5e-5 on the bench workload — inside the 1e-4
 * contract for weights of ordinary size but without the 2x margin f16x3 keeps everywhere, hence opt-in.
 * F16F8 (forward / inference only) = f16 main term + the two cross terms of the hi/lo split on v_mfma_f32_32x32x16_fp8_fp8 (e4m3): the
 * instruction count and operand bytes of F16X3 at lower power (the engine is power-limited: ~8 % faster); measured end-to-end |dRGB| vs the
 * oracle 2e-6.  Its operand stream scales the weights by 2^14: a NerfMLP weight of magnitude >= 3.99 raises a flag in rnerf_nerfmlp_pack, and
 * every rnerf_nerfmlp_forward launch then steps aside for the F16X3 launch queued behind it (the F16F8 packed buffer carries both streams):
 * a per-launch fallback decided on the device, F16X3's bits, no host round trip.  Own packed stream: pack with the precision you run.
 * Round 6: a row with an operand of magnitude >= 448 (e4m3's largest value: fp8(x) of the W_lo cross term would be clamped) is given up like
 * a row out of f16's range and recomputed by the range-safe second pass.  Accuracy depends on the weights: 2e-6 |dRGB| on glorot-initialised
 * networks, 2e-4 with hidden kernels x 1.5 and N(0, 0.3) biases (outside the 1e-4 contract): an opt-in precision, not a default.
 * Range of the f16-based modes.  The forward watches the largest f16 operand it forms per row; a weight of magnitude >= 256 (2^8-scaled
 * streams) or a hidden activation above f16's 65504 makes the first pass give the row up (NaN), never return a plausible wrong colour.
 * EVALUATION (rnerf_nerfmlp_forward with F16X3 / F16X2 / F16F8 / F16, hence rnerf_forward): every launch is followed on the device by a range-safe
 * second pass in BF16X3 (fp32's exponent range; its stream sits behind the others in the packed buffer) that recomputes exactly the rows
 * the first pass gave up on and touches no other row — the reference's fp32 nn.Dense (rnerf/model_utils.py:58-89) is finite there, and so is
 * this; without such a row the pass reads the outputs once (~5 us) and the first pass's bits stand.  The
 * TRAINING forward (rnerf_nerfmlp_forward_train) has no per-row second pass — the saved f16 operands of the backward cannot represent such a
 * row: it stays NaN, reaches the non-finite-gradient count of rnerf_adam_update (scratch[3]), the update is skipped
 * (rnerf_adam_cfg.skip_nonfinite) and the STEP is re-run in BF16X3 + backward BF16, the range-safe training arithmetic. */
enum rnerf_precision {
  RNERF_PREC_F32 = 0,
  RNERF_PREC_F16X3 = 1,
  RNERF_PREC_BF16X3 = 2,
  RNERF_PREC_F16 = 3,
  RNERF_PREC_BF16 = 4,
  RNERF_PREC_F16X2 = 5,
  RNERF_PREC_F16F8 = 6
};

/* Arithmetic of the NerfMLP backward (dgrad + wgrad).  The reference differentiates in fp32 (train.py:164).
 *   BF16  : gradients rounded to bf16 (8-bit significand), saved activations rounded to bf16 in the wgrad: 1 MFMA per product.
 *   F16   : every row's gradient chain is normalised by a power of two m_row ~ max |d raw[row]| (the chain is linear in d raw[row], so
 *           the normalised values fit f16's range whatever the loss scale); f16 operands (11-bit significand, the class of the TF32
 *           tensor-core arithmetic XLA uses for fp32 matmuls on the authors' Ampere GPU): 1 MFMA per product, same HBM traffic as BF16.
 *   F16X3 : as F16 with hi + lo parts of the saved activations and of every gradient (22 bits), 3 MFMAs per product: fp32-grade
 *           (<= 1e-5 of the largest gradient entry against float64); twice the saved bytes.
 *   F16X3_LO8 (round 6): F16X3 with the lo plane of every saved activation and of every gradient STORED as one e4m3 byte per value
 *           (scaled by a fixed power of two, clamped instead of overflowing) and decoded back to f16 inside the wgrad: the same three f16
 *           MFMAs per product with the exact f16 hi parts in both cross terms, three quarters of the bytes of every operand stream of
 *           the step (hi 2 B + lo 1 B per value).  The dgrad chain itself runs on the full hi + lo f16 parts (registers); only what the
 *           wgrad reads is 8-bit.  An 11 + 4 bit significand per operand: measured gradient error vs float64 in DESIGN.md §3.3.
 *           Buffer sizes are those of F16X3 (the lo planes use half of their region). */
enum rnerf_backward {
  RNERF_BWD_BF16 = 0,
  RNERF_BWD_F16 = 1,
  RNERF_BWD_F16X3 = 2,   /* hi + lo f16 planes, 3 MFMAs per product */
  RNERF_BWD_F16X2 = 2,   /* the name of versions <= 1 (two planes); same value */
  RNERF_BWD_F16X3_LO8 = 4   /* hi f16 plane + lo e4m3 plane (3 is an internal dgrad variant) */
};

/* Voxel grid geometry: reference VoxMLP.ndim/nmin/nmax (rnerf/ior_utils.py:124-144).  Doubles, because the
 * reference derives ndelta = (nmax-nmin)/(ndim-1) in Python doubles before it meets float32 data. */
typedef struct rnerf_grid {
  int32_t dims[3];
  double nmin[3];
  double nmax[3];
  int32_t layout;   /* enum rnerf_table_layout: the memory order of the float4 table built for / read with this grid */
} rnerf_grid;

/* Memory order of the (n, grad n) table.  REFERENCE = flat index x*Gy*Gz + y*Gz + z, x slowest (rnerf/ior_utils.py:161,214 — the order the
 * reference indexes with).  BRICKS = 2x2x2 bricks of 128 bytes, bricks x-major: entry (x, y, z) lives at
 *   (((x>>1)*By + (y>>1))*Bz + (z>>1))*8 + (x&1)*4 + (y&1)*2 + (z&1),   B* = ceil(G* / 2)
 * so the 8 corners of a trilinear lookup in an even-aligned cell are ONE 128-byte line and a bent ray meets ~40 % fewer new lines per step
 * (SURVEY 8f N2 "Morton / brick relayout"; measured in profiles/r04/march_time.txt).  Values and indices are the reference's either way:
 * only addresses differ.  Every entry point that takes (table, grid) reads the table in grid->layout; rnerf_grid_build_table writes it so. */
enum rnerf_table_layout {
  RNERF_TABLE_REFERENCE = 0,
  RNERF_TABLE_BRICKS = 1
};
/* floats a table of this grid / layout occupies (REFERENCE: 4 G^3; BRICKS: 32 per brick, odd dimensions padded to whole bricks) */
size_t rnerf_grid_table_floats(const rnerf_grid* g);

/* Sizes of the flat fp32 parameter buffers (flax creation order Dense_0.. ; per layer kernel[in][out]
 * row-major followed by bias[out]).  NerfMLP: rnerf/model_utils.py:30-90, MLP: :93-140. */
#define RNERF_NERFMLP_PARAMS 595844
#define RNERF_BKGDMLP_PARAMS 56963
#define RNERF_SO3MLP_PARAMS 65411   /* so3_mlp: 60->128->128->128(+60)->128->3 (rnerf/ior_utils.py:148-152) */

const char* rnerf_last_error(void);
int rnerf_version(void);
/* Number of compute units of the current device (for host-side sizing); <0 on error. */
int rnerf_device_cus(void);

/* ---- G1: Gaussian prefilter of the IoR grid.  Replaces ior_utils.conv3d_normal (rnerf/ior_utils.py:327-363).
 * src/dst/tmp: float[dims0*dims1*dims2], x slowest.  Separable evaluation of the same normalised kernel. */
int rnerf_grid_prefilter(const float* src, float* dst, float* tmp, const int32_t dims[3], int ksize, double ksigma,
                         void* stream);

/* ---- G2: n + central-difference gradient table.  Replaces VoxMLP.setup/_compute_grad
 * (rnerf/ior_utils.py:139-172).  table: float4[G^3] = (n, dn/dx, dn/dy, dn/dz). */
int rnerf_grid_build_table(const float* grid, float* table, const rnerf_grid* g, void* stream);

/* ---- G3: trilinear lookup with clamp-to-edge.  Replaces VoxMLP._linear3 (rnerf/ior_utils.py:188-223).
 * pts: float[n][3]; out: float[n][4]; idx (nullable): int32[n][6] = clamped x0,x1,y0,y1,z0,z1 (debug tap). */
int rnerf_grid_query(const float* table, const rnerf_grid* g, const float* pts, int64_t n, float* out, int32_t* idx,
                     void* stream);

/* ---- E1/E2/E3: eikonal march.  Replaces PathSampler.__call__ + OneEikonalStep.__call__
 * (rnerf/eikonal_utils.py:29-49,100-124) with stage="radiance*" and math_utils.safe_l2_normalize
 * (rnerf/math_utils.py:6-12).  num_nodes = N_c*P, step = (far-near)/(num_nodes-1) (rnerf/models.py:121-122).
 * origins, viewdirs: float[B][3].  path_pd, path_dr: float4[num_nodes][B] node records (node k = state before
 * step k).  path_ior (nullable): float4[num_nodes][B] = (n, grad n) at node k.  vox (nullable): int32
 * [num_nodes][B][6] clamped voxel indices (debug tap for the bit-exact test). */
int rnerf_march(const float* table, const rnerf_grid* g, const float* origins, const float* viewdirs, int32_t B,
                double near, double far, int32_t num_nodes, float* path_pd, float* path_dr, float* path_ior,
                int32_t* vox, void* stream);
/* rnerf_march that records the sampled nodes only (appended; RNERF_VERSION stays 4).  sample_nodes: device int32[num_nodes / num_path],
 * one node per group of num_path consecutive nodes (the jitter of rnerf_rng_forward); node k is recorded where
 * sample_nodes[k / num_path] == k, with the bits rnerf_march writes there (position, normalised direction, distance), and every other
 * record of path_pd / path_dr is left as it was: only a consumer that reads the path through this very array may use it (a flat model:
 * num_fine == 0).  num_nodes must be a multiple of num_path.  sample_nodes == NULL: every node, as rnerf_march. */
int rnerf_march_sparse(const float* table, const rnerf_grid* g, const float* origins, const float* viewdirs, int32_t B,
                       double near, double far, int32_t num_nodes, float* path_pd, float* path_dr,
                       const int32_t* sample_nodes, int32_t num_path, void* stream);

/* ---- N1 weights: pack a flat fp32 NerfMLP parameter buffer into the MFMA operand stream of `precision`. */
size_t rnerf_nerfmlp_packed_bytes(int precision);
int rnerf_nerfmlp_pack(const float* params, int precision, void* packed, void* stream);

/* ---- P1 + N1: positional encoding + NerfMLP over sample rows.  Replaces model_utils.pos_enc
 * (rnerf/model_utils.py:187-214) and NerfMLP.__call__ (:30-90) as called at rnerf/models.py:257,289,305,394,426,441.
 * Rows are sample-major: row = s*B + b.  If node_of_sample != NULL (int32[S], device) the record of row (s,b) is
 * read at node_of_sample[s]*B + b (coarse pass reading the path record through the jitter); otherwise at s*B + b.
 * packed: the buffer written by rnerf_nerfmlp_pack (weight stream + fp32 biases and sigma/rgb heads).
 * out_raw: float4[S*B] = (raw_r, raw_g, raw_b, raw_sigma) before activation.
 * max_workgroups: cap of the persistent grid (0 = one workgroup per CU).  The kernel owns a whole CU (512 VGPRs, 160 KiB LDS); a
 * caller that marches the NEXT ray batch on another stream leaves a few CUs free for it with this argument (no library state). */
int rnerf_nerfmlp_forward(const void* packed, int precision, const float* rows_pd, const float* rows_dr,
                          const int32_t* node_of_sample, int32_t S, int32_t B, float* out_raw, int32_t max_workgroups, void* stream);

/* ---- P1 + N2: background MLP on one direction per ray.  Replaces bkgd_mlp(viewdirs_enc[:, -1:]) +
 * rgb activation (rnerf/models.py:303,336-337) and NerfModel.forward_envmap (:181-191).
 * dirs: float[n][dir_stride] (dir_stride 3 or 4), out_rgb: float[n][3] after sigmoid*(1+2p)-p. */
int rnerf_bkgd_forward(const float* params, const float* dirs, int32_t dir_stride, int64_t n, double rgb_padding,
                       float* out_rgb, void* stream);

/* ---- V1: activations + alpha compositing.  Replaces rgb/sigma activation (rnerf/models.py:334-338) and
 * model_utils.volumetric_rendering (rnerf/model_utils.py:247-309).  Row addressing as rnerf_nerfmlp_forward.
 * bkgd: float[B][3].  Outputs: rgb float[B][3], dist float[B], acc float[B], trans float[B],
 * trans_bkgd float[B][3]; weights (nullable) float[S][B]; alpha (nullable) float[S][B].
 * mask_mode / bbox (host double[6] = min xyz, max xyz): the bd_cut_dist masks of rnerf/models.py:479-524 — 0 none,
 * 1: density_delta *= mask_bbox (1 up to the last sample inside the box), 2: density_delta *= 1 - mask_bbox;
 * 3: use_mask_bbox (rnerf/models.py:261-271,398-408): density_delta *= 1[this sample is inside the box]. */
int rnerf_composite(const float* raw, const float* rows_pd, const float* rows_dr, const int32_t* node_of_sample,
                    int32_t S, int32_t B, const float* bkgd, int white_bkgd, double rgb_padding, double sigma_bias,
                    float* rgb, float* dist, float* acc, float* trans, float* trans_bkgd, float* weights,
                    float* alpha, int mask_mode, const double* bbox, void* stream);

/* ---- S1 + S2: PDF resampling along the bent path.  Replaces sorted_piecewise_constant_pdf and sample_pdf
 * (rnerf/model_utils.py:312-435) as called at rnerf/models.py:371-384.
 * jitter: int32[S] coarse node indices; weights: float[S][B] coarse weights; u: the uniform draws,
 * float[num_fine][B] if u_per_ray else float[num_fine] shared by all rays (randomized=False: linspace(0, 1-eps32, F),
 * rnerf/model_utils.py:355-356).  u must be non-decreasing along the sample axis (true for both reference branches).
 * Outputs (S+num_fine rows per ray, sample-major): rows_pd/rows_dr records, node_idx (nullable) int32[S+F][B]
 * the searchsorted node index (bit-exact contract).  scratch: float[S+num_fine][B] (the merged depths). */
int rnerf_resample(const float* path_pd, const float* path_dr, int32_t num_nodes, int32_t B, const int32_t* jitter,
                   int32_t S, const float* weights, const float* u, int32_t u_per_ray, int32_t num_fine, float* rows_pd,
                   float* rows_dr, int32_t* node_idx, float* scratch, void* stream);

/* ---- S1 (randomized=True): the stratified uniform draws of sorted_piecewise_constant_pdf, rnerf/model_utils.py:345-354:
 * u = min(arange(F)/F + jax.random.uniform(key, [B,F], maxval=1/F-eps), 1-eps) with jax's threefry2x32 bit stream.
 * key: HOST uint32[2]; u: device float[num_fine][B] (the layout rnerf_resample takes with u_per_ray = 1). */
int rnerf_stratified_u(const uint32_t* key, int32_t B, int32_t num_fine, float* u, void* stream);

/* ---- the voxeliser.  Replaces voxelize_mesh.py:54-106 (pysdf point-in-mesh in a Python loop over G^3 voxels):
 * out[i][j][k] = mean over the K^3 sub-samples c + linspace(-1,1,K)^3 * pitch of (inside ? ior_inside : ior_outside), x slowest.
 * verts: device double[V][3]; faces: device int32[F][3]; bin_start int32[num_bins^2 + 1] / bin_tris: CSR lists of the triangles
 * overlapping each cell of a num_bins x num_bins grid over the xy plane (cell index bx * num_bins + by), built by the host;
 * bin_origin_size: HOST double[4] = (x0, y0, cell size x, cell size y).  Inside = odd number of surface crossings along +z
 * (top-left rule on shared edges, fp64).  count: device int32[G^3] scratch; overflow: device int32[1], non-zero if a column met
 * more than 96 crossings (result then invalid). */
int rnerf_voxelize(const double* verts, const int32_t* faces, const int32_t* bin_start, const int32_t* bin_tris, int32_t num_bins,
                   const double* bin_origin_size, const rnerf_grid* g, int32_t num_samples, double ior_inside, double ior_outside,
                   int32_t* count, float* out, int32_t* overflow, void* stream);

/* Robust containment for meshes that are NOT watertight (pysdf casts one parity ray per point in a randomly rotated frame,
 * sdf/src/sdf.cpp:156-168,270-322; a single ray through a hole misclassifies the point): three passes of the same column test along
 * +z, +x, +y, then a per-sample majority.
 *   rnerf_voxelize_samples : as rnerf_voxelize, but writes the inside flag of every sample: inside uint8[GK][GK][GK], GK = G * K, indexed
 *                            [x sample][y sample][z sample] of the coordinates it was GIVEN.  The caller runs it three times with the mesh
 *                            and the grid axes rotated: (x, y, z), (y, z, x), (z, x, y) (samplenerfro_amd/voxelize.py: robust=True).
 *   rnerf_voxelize_majority: in_z / in_x / in_y = the outputs of those three passes; count int32[G^3] = samples with >= 2 of 3 votes. */
int rnerf_voxelize_samples(const double* verts, const int32_t* faces, const int32_t* bin_start, const int32_t* bin_tris, int32_t num_bins,
                           const double* bin_origin_size, const rnerf_grid* g, int32_t num_samples, uint8_t* inside, int32_t* overflow, void* stream);
int rnerf_voxelize_majority(const uint8_t* in_z, const uint8_t* in_x, const uint8_t* in_y, int32_t num_voxels, int32_t num_samples,
                            double ior_inside, double ior_outside, int32_t* count, float* out, void* stream);

/* ---- G4 + P2: VoxMLP.__call__ (rnerf/ior_utils.py:269-312, shipped gin: annealed, use_residual, use_direct_output):
 * (n, grad n) by trilinear lookup and pred_grad = grad n rotated (Rodrigues) by the axis-angle so3_mlp(annealed_pos_enc(x)).
 * so3_params: device float[RNERF_SO3MLP_PARAMS] (flax order); window10: HOST float[10] = cosine_easing_window(0, 9, 10,
 * annealed_alpha * 10) (rnerf/model_utils.py:218-233); pts: device float[n][3]; out4: float4[n] = (n, grad n); pred_grad: float[n][3].
 * condition (nullable, device float[n][3]): rotate this vector instead of the looked-up gradient = VoxMLP.wrapper_grad_mlp
 * (rnerf/ior_utils.py:225-267), the building block of E4 compute_normal_loss_and_smooth (rnerf/eikonal_utils.py:84-98). */
int rnerf_so3_query(const float* table, const rnerf_grid* g, const float* so3_params, const float* window10, const float* pts,
                    const float* condition, int64_t n, float* out4, float* pred_grad, void* stream);

/* ---- E1/E2 with stage "all*": the march with grad = where(|grad n| > 1e-3, pred_grad, grad n) (rnerf/eikonal_utils.py:34-39).
 * Outputs as rnerf_march (path_ior nullable).  so3_packed: device scratch of rnerf_so3_packed_bytes() bytes — the call packs the so3
 * parameters into the f16 hi + lo A-operand stream of the in-march MLP (3 x v_mfma_f32_16x16x32_f16 per tile, fp32 accumulate).
 * ray_order (nullable): int32[B], a permutation of the rays: workgroup i marches rays ray_order[16 i .. 16 i + 15] (a group of 16
 * evaluates the MLP whenever ANY of its rays is inside the boundary shell, so rays with similar shell intervals should share a group).
 * Every record is written at the ray's own index: the order changes no output.
 * Grid size limit of every marching entry point: the table is addressed with 32-bit byte offsets and 24-bit strides —
 * dims[0] * dims[1] * dims[2] * 16 B < 4 GiB in all of them; rnerf_march_all / rnerf_march_all_train / rnerf_march_adjoint (and
 * rnerf_march on a BRICKS table) need the stride of TWO x-planes below 2^24: dims[1] * dims[2] * 32 < 2^24 (reference order;
 * ceil(dims[1]/2) * ceil(dims[2]/2) * 128 < 2^24 for bricks); rnerf_march on a REFERENCE-order table needs only dims[1] * dims[2] * 16 < 2^24.
 * Cubic grids up to 645^3 in reference order and 644^3 in bricks (odd dimensions are padded to whole bricks) pass every check (every
 * shipped config: 128^3 .. 512^3); larger grids are rejected with RNERF_ERR_ARG ("grid too large"), never mis-addressed. */
size_t rnerf_so3_packed_bytes(void);
int rnerf_march_all(const float* table, const rnerf_grid* g, const float* so3_params, void* so3_packed, const float* window10, const float* origins,
                    const float* viewdirs, int32_t B, double near, double far, int32_t num_nodes, float* path_pd, float* path_dr,
                    float* path_ior, const int32_t* ray_order, void* stream);

/* ---- pinhole ray generation on the device.  Replaces Dataset._generate_rays (rnerf/datasets.py:216-242, Blender
 * model: opencv = 0, fx = fy = focal, cx = W/2, cy = H/2) and the OpenCV variant (:486-518: opencv = 1, fx, fy, cx, cy from cam_mat),
 * for rows [row0, row0+rows) of one view.  camtoworld: HOST float[3][4] (row-major, rotation | translation).
 * origins / directions (nullable) / viewdirs: device float[rows][W][3]. */
int rnerf_generate_rays(const float* camtoworld, int32_t opencv, double fx, double fy, double cx, double cy, double pixel_center,
                        int32_t W, int32_t row0, int32_t rows, float* origins, float* directions, float* viewdirs, void* stream);

/* ---- the gather half of Dataset._next_train (rnerf/datasets.py:151-176: `batch_pixels = self.images[...][ray_indices]`,
 * `batch_rays = namedtuple_map(lambda r: r[...][ray_indices], self.rays)`; :178-197 for the env-map patch) on the device.  The training
 * views stay resident: camtoworlds DEVICE float[n_img][3][4], images DEVICE float[n_img][H][W][channels] (nullable together with
 * `pixels`: rays only, the env-map patch).  ray_indices: DEVICE int64[B], flat `image * H * W + row * W + column` — "all_images" batching
 * indexes the concatenation of all views exactly like that (datasets.py:131-136), "single_image" adds image_index * H * W on the host.  The
 * rays of the drawn pixels are generated on the fly by the arithmetic of rnerf_generate_rays (same camera arguments: bit-identical to
 * indexing the reference's ray arrays); no ray array is ever stored.  bad_count: DEVICE int32, incremented for every index outside
 * [0, n_img * H * W) (such a ray reads pixel 0; the caller zeroes and checks the counter).  origins / directions (nullable) / viewdirs:
 * float[B][3]; pixels: float[B][channels].  The index DRAW stays the caller's (the reference draws with numpy's global generator,
 * datasets.py:154-169: a host sequence this library does not restate). */
int rnerf_sample_batch(const float* camtoworlds, int32_t n_img, int32_t opencv, double fx, double fy, double cx, double cy, double pixel_center,
                       int32_t W, int32_t H, const float* images, int32_t channels, const int64_t* ray_indices, int32_t B, float* origins,
                       float* directions, float* viewdirs, float* pixels, int32_t* bad_count, void* stream);

/* ---- mip-style integrated positional encoding along the curved ray.  Replaces mip.cast_rays(t_vals, ray_pos_c, ray_dir_c,
 * rays.radii, "cone", near) + mip.integrated_pos_enc(samples, min_deg, max_deg) (rnerf/mip.py:26-57,60-91,116-175) as the commented call sites
 * of the reference use them (rnerf/models.py:249-254,386-391): the S samples of a ray (row addressing as rnerf_nerfmlp_forward; depths in
 * pd.w) are the axes of conical frusta between consecutive depths (the last one 1e-3 long); each becomes a diagonal Gaussian whose mean is
 * accumulated along the bent path.  radii: float[B] (Rays.radii).  Outputs (each nullable, sample-major): out_mean4 float4[S][B] =
 * (mean xyz, t_mean), out_cov4 float4[S][B] = (diagonal covariance xyz, t_var), out_enc float[S][B][6 (max_deg - min_deg)] =
 * exp(-var/2) sin(.) of [y, y + pi/2], y = mean * 2^deg degree-major (no identity features). */
int rnerf_integrated_pos_enc(const float* rows_pd, const float* rows_dr, const int32_t* node_of_sample, int32_t S, int32_t B, const float* radii,
                             double near, int32_t min_deg, int32_t max_deg, float* out_mean4, float* out_cov4, float* out_enc, void* stream);

/* ---- T1 (loss): the reductions of train_step.loss_fn (train.py:89-92,105) for stage "radiance*".
 * rgb_c (nullable, N_f == 0), rgb_f: float[B][3]; trans_f: float[B]; trans_bkgd_f, pixels: float[B][3].
 * sums: float[4] (device) = { sum (rgb_f-pix)^2, sum (rgb_c-pix)^2, sum mask*|trans_bkgd_f-pix|, sum mask },
 * mask = trans_f > 0.5.  loss = sums0/(3B) + sums1/(3B) + bg_weight*1[alpha>0]*sums2/(sums3+1) + ... */
int rnerf_loss_reduce(const float* rgb_c, const float* rgb_f, const float* trans_f, const float* trans_bkgd_f,
                      const float* pixels, int32_t B, float* sums, void* stream);

/* ---- T1 (scalar tail of loss_fn).  rnerf_env_smooth_backward: the env-map smoothness term of train.py:127-130 on the patch
 * rgb_env float[ps][ps][3]: d_out float[ps*ps][3] = grad_scale * d mean(0.5 dv^2 + 0.5 dh^2) / d rgb_env; loss_sum (device,
 * rnerf_env_smooth_sum_floats(ps) floats, need not be cleared) receives the un-normalised sum as one partial per workgroup behind 4 reserved
 * floats — rnerf_train_stats (env_loss_sum = this buffer) adds them in index order: no float atomics, the same bits from run to run (round 4;
 * the same holds for rnerf_theta_sumsq, one workgroup with a fixed summation order).  rnerf_train_stats: utils.Stats scalars (train.py:147-162) into stats8 (device float[8], zeroed by the
 * caller): [0] loss, [1] loss_c, [2] loss_bg = bg_scale * sums2 / (sums3 + 1) with bg_scale = bg_weight * 1[annealed_alpha > 0], [3] loss_bg_smooth, [4] weight_l2 = (sum theta^2 + frozen_sq) / n_all, [6] psnr,
 * [7] psnr_c; sums = rnerf_loss_reduce's output. */
size_t rnerf_env_smooth_sum_floats(int32_t ps);
int rnerf_env_smooth_backward(const float* rgb_env, int32_t ps, double grad_scale, float* d_out, float* loss_sum, void* stream);
int rnerf_train_stats(const float* sums, int32_t B, int32_t two_levels, double bg_scale, const float* env_loss_sum, int32_t ps, double env_on,
                      const float* theta, int64_t n_theta, double frozen_sq, int64_t n_all, float* stats8, void* stream);
/* rnerf_train_stats in two parts (the sum of squares of theta does not depend on the step's data and may run anywhere before the scalars):
 * rnerf_theta_sumsq writes sum theta^2 to stats8[5]; rnerf_train_stats with theta == NULL then only forms the scalars. */
int rnerf_theta_sumsq(const float* theta, int64_t n_theta, float* stats8, void* stream);

/* ---- T1 (backward of V1 + activations): d loss / d raw of one level, replacing jax.value_and_grad through
 * volumetric_rendering and the rgb/sigma activations (rnerf/model_utils.py:247-309, rnerf/models.py:334-338; train.py:164).
 * rgb: this level's comp_rgb float[B][3]; mse_scale = 2/(3B); bg_scale = bg_weight*1[annealed_alpha>0] for the level
 * that carries loss_bg (the last one), 0 otherwise (then trans/trans_bkgd/sums may be NULL).
 * d_raw: float4[S][B]; d_bkgd: float[B][3] gradient w.r.t. the activated background colour (accumulated if
 * accumulate_bkgd != 0: both levels composite over the coarse pass's bkgd, rnerf/models.py:468-476).
 * white_bkgd: comp_rgb carried the + (1 - acc) term of rnerf/model_utils.py:307-308.
 * mask_mode / bbox (host double[6] = min xyz, max xyz; NULL with mask_mode 0): 1 = the level's trans / trans_bkgd are the bd_cut_dist pair of
 * rnerf/models.py:479-524 (trans = mask_mode-1 transmittance, trans_bkgd = trans * mask_mode-2 colour over bkgd); 3 = the level was rendered
 * with use_mask_bbox (rnerf/models.py:261-271,398-408: density_delta *= 1[sample inside the box]), the gradient carries the same mask. */
int rnerf_composite_backward(const float* raw, const float* rows_pd, const float* rows_dr, const int32_t* node_of_sample,
                             int32_t S, int32_t B, const float* bkgd, double rgb_padding, double sigma_bias, const float* rgb,
                             const float* pixels, const float* trans, const float* trans_bkgd, const float* sums,
                             double mse_scale, double bg_scale, float* d_raw, float* d_bkgd, int accumulate_bkgd, int white_bkgd,
                             int mask_mode, const double* bbox, void* stream);

/* ---- T1 (backward of P1+N1): gradient of the NerfMLP parameters, replacing jax.value_and_grad through
 * NerfMLP.__call__ (train.py:164; rnerf/model_utils.py:30-90).  `backward` is an enum rnerf_backward, the same in all calls of a step.
 *   rnerf_nerfmlp_forward_train : as rnerf_nerfmlp_forward — precision F16X3 (the fp32-grade default), F16 with backward F16 / BF16 (the
 *       single-pass training arithmetic: one MFMA per product, a labelled bench leg), or BF16X3 with backward BF16 (the RANGE-SAFE training
 *       arithmetic: fp32's exponent range in the forward, the saved operands and the gradients; 16-bit forward products, 8-bit gradients —
 *       what a step whose f16-based run met a row outside f16's range is re-run in); the dgrad / wgrad calls of the step take the same
 *       precision; bf16 / f16x2 / f16f8 are inference precisions — and keeps
 *       the 16-bit operands of every layer in `save` (rnerf_nerfmlp_save_bytes(S*B, backward) bytes; F16X3 backward: hi and lo parts);
 *   rnerf_nerfmlp_pack_bwd : transposed weight stream of the dgrad chain (rnerf_nerfmlp_bwd_packed_bytes() bytes);
 *   rnerf_nerfmlp_dgrad : d_raw float4[rows] (d loss / d raw rgb, sigma) -> dy (rnerf_nerfmlp_dy_bytes(rows, backward) bytes), the
 *       gradients w.r.t. every layer's pre-activation output (F16 modes: normalised per row, + the row scales);
 *   rnerf_nerfmlp_wgrad : (save, dy) -> grads float[RNERF_NERFMLP_PARAMS] in the flat parameter order (every entry is
 *       overwritten); workspace: rnerf_nerfmlp_wgrad_workspace_bytes() bytes. */
size_t rnerf_nerfmlp_save_bytes(int64_t rows, int backward);
size_t rnerf_nerfmlp_dy_bytes(int64_t rows, int backward);
size_t rnerf_nerfmlp_bwd_packed_bytes(void);
size_t rnerf_nerfmlp_wgrad_workspace_bytes(void);
int rnerf_nerfmlp_forward_train(const void* packed, int precision, const float* rows_pd, const float* rows_dr,
                                const int32_t* node_of_sample, int32_t S, int32_t B, float* out_raw, void* save, int backward,
                                int32_t max_workgroups /* as rnerf_nerfmlp_forward: 0 = one workgroup per CU */, void* stream);
int rnerf_nerfmlp_pack_bwd(const float* params, int backward, void* packed_bwd, void* stream);
int rnerf_nerfmlp_dgrad(const void* packed_bwd, const void* packed_fwd, int fwd_precision, int backward, const void* save, const float* d_raw,
                        int64_t rows, void* dy, void* stream);
int rnerf_nerfmlp_wgrad(int fwd_precision, int backward, const void* save, const void* dy, int64_t rows, float* grads, void* workspace,
                        void* stream);

/* ---- T1 (backward of P1+N2): the background MLP, exact fp32 on the matrix cores (its forward: f16 hi + lo, like the NerfMLP's f16x3).
 * rnerf_bkgd_forward_train = rnerf_bkgd_forward + `save` (rnerf_bkgd_save_bytes(n) bytes).
 * rnerf_bkgd_backward: d_out float[n][3] (d loss / d activated bkgd colour) -> ACCUMULATES into grads
 * float[RNERF_BKGDMLP_PARAMS] (the caller zeroes it once per step: the per-ray bkgd and the env-map patch, train.py:127-130,
 * both add to it); dy: scratch of rnerf_bkgd_dy_bytes(n) bytes.  d_dirs (nullable): float4[n], d loss / d direction through pos_enc(dir)
 * (stage "all*": the direction of the last coarse sample is a function of the so3 parameters). */
size_t rnerf_bkgd_save_bytes(int64_t n);
size_t rnerf_bkgd_dy_bytes(int64_t n);
int rnerf_bkgd_forward_train(const float* params, const float* dirs, int32_t dir_stride, int64_t n, double rgb_padding,
                             float* out_rgb, void* save, void* stream);
int rnerf_bkgd_backward(const float* params, const void* save, const float* d_out, int64_t n, double rgb_padding, void* dy,
                        float* grads, float* d_dirs, void* stream);

/* ---- training of stage "all*" — jax.value_and_grad (train.py:164) through the N-step eikonal recurrence
 * (rnerf/eikonal_utils.py:29-49,100-124) and through so3_mlp + the Rodrigues rotation (rnerf/ior_utils.py:269-312), with path_sampler
 * trainable (train.py:302-310).  The state of the recurrence is 6 numbers per ray, so its adjoint is a reverse scan with 3x3 Jacobians;
 * everything that involves the so3 MLP runs as parallel batches over the (ray, node) PAIRS at which pred_grad was selected:
 *   rnerf_march_all_train  : rnerf_march_all + the record the backward needs: path_rdn float4[N][B] = (raw direction, n) per node, and
 *                            the compacted pairs (pair_count device int32, zeroed by the call; pair_id int32[cap][2] = (ray, node);
 *                            pair_x / pair_g float4[cap] = position / looked-up gradient; pair_of_node int32[N][B], -1 = none);
 *   rnerf_so3_forward_train: so3_mlp on pts4 float4[n] -> save (rnerf_so3_save_bytes(n): fp32 [enc n x 60][X1..X4 n x 128][raw float4[n], at float offset
 *                            572 n], then the layers' ReLU sign bits uint32[4][n][4], which is all the dgrad chain reads of the activations);
 *   rnerf_so3_backward     : cotangents d_raw4 float4[nb] -> dx4 float4[nb] (nullable, d / d point) and, if grads != NULL (nb == n_save),
 *                            grads float[RNERF_SO3MLP_PARAMS] += ...; row i uses the saved activations of row i % n_save, so the three
 *                            unit cotangents of every point run as one batch of 3 n_save rows (the rows of J = d raw / d x);
 *                            dy (rnerf_so3_dy_bytes(nb)) is scratch for the parameter gradient: written only when grads != NULL;
 *   rnerf_so3_pair_jacobian: per pair A = d grad / d position (P J + (d pred / d g) G, G = d g / d x of the trilinear interpolant) and
 *                            P = d pred / d raw, float[np][12] each (9 used, row-major);
 *   rnerf_march_adjoint    : the reverse scan; a_pos / a_dir float4[S][B] = d loss / d (position, normalised direction) of the coarse
 *                            samples, sample_of_node int32[N] (-1 = the node is no sample) -> v4 float4[np], the cotangent of raw per pair;
 *   rnerf_nerfmlp_input_grad: d loss / d (position, direction) of every row of a NerfMLP level from the dgrad's dy buffer (F16 modes):
 *                            through pos_enc into Dense_0, the skip concat of Dense_5 and the view layer Dense_10. */
int rnerf_march_all_train(const float* table, const rnerf_grid* g, const float* so3_params, void* so3_packed, const float* window10, const float* origins,
                          const float* viewdirs, int32_t B, double near, double far, int32_t num_nodes, float* path_pd, float* path_dr,
                          float* path_rdn, int32_t* pair_count, int32_t pair_cap, int32_t* pair_id, float* pair_x, float* pair_g,
                          int32_t* pair_of_node, const int32_t* ray_order, void* stream);
size_t rnerf_so3_save_bytes(int64_t n);
size_t rnerf_so3_dy_bytes(int64_t nb);
int rnerf_so3_forward_train(const float* so3_params, const float* window10, const float* pts4, int64_t n, void* save, void* stream);
int rnerf_so3_backward(const float* so3_params, const float* window10, const float* pts4, const void* save, int64_t n_save, const float* d_raw4,
                       int64_t nb, void* dy, float* dx4, float* grads, void* stream);
int rnerf_so3_pair_jacobian(const float* table, const rnerf_grid* g, const float* pair_x, const float* pair_g, const float* raw4, const float* J4,
                            int64_t np, float* A12, float* P12, void* stream);
int rnerf_march_adjoint(const float* table, const rnerf_grid* g, const float* path_pd, const float* path_rdn, const int32_t* pair_of_node,
                        const float* A12, const float* P12, const float* a_pos, const float* a_dir, const int32_t* sample_of_node, int32_t B,
                        double near, double far, int32_t num_nodes, float* v4, void* stream);
int rnerf_nerfmlp_input_grad(const float* params, int backward, const void* dy, const float* rows_pd, const float* rows_dr,
                             const int32_t* node_of_sample, int32_t S, int32_t B, float* d_pos4, float* d_dir4, void* stream);

/* ====================================================================================================================================
 * Whole-path entry points ("rnerf_forward / rnerf_backward + a workspace-size query").  They sequence the stage launchers
 * above exactly as NerfModel.__call__ (rnerf/models.py:220-535) and train_step (train.py:58-183) do, on ONE stream, from caller-owned
 * device buffers, with no host round trip in between — so a host in any language drives the path with one call per ray batch, and a
 * whole step can be captured into one launch graph (rnerf_graph_*).  Every random number of the path comes from DEVICE-resident
 * jax.random keys (rnerf_rng_*), which is what makes the step capturable.
 * ==================================================================================================================================== */

/* What NerfModel closes over (attributes rnerf/models.py:42-90, setup :91-137).  Plain data; pointers are device pointers. */
typedef struct rnerf_model {
  const float* table;          /* float4[G^3] written by rnerf_grid_build_table (VoxMLP.setup, rnerf/ior_utils.py:139-172) */
  rnerf_grid grid;
  double near, far;            /* rnerf/models.py:122 */
  int32_t num_coarse;          /* N_c  (num_coarse_samples) */
  int32_t num_fine;            /* N_f  (num_fine_samples; 0 = single level, rnerf/models.py:368) */
  int32_t num_path;            /* P    (num_path_samples): N = N_c * P eikonal nodes */
  int32_t precision;           /* enum rnerf_precision of packed_coarse / packed_fine */
  int32_t white_bkgd;          /* rnerf/model_utils.py:307-308 */
  int32_t bd_cut;              /* 1: the fine level's trans / trans_rgb_bkgd are the bd_cut_dist pair (rnerf/models.py:479-524);
                                * 2: use_mask_bbox (rnerf/models.py:261-271,398-408): both levels keep density only at samples inside bd_cut_bbox
                                *    (the reference's box is the grid's nmin / nmax) */
  double rgb_padding, sigma_bias;   /* rnerf/models.py:78-79 */
  double bd_cut_bbox[6];       /* min xyz, max xyz (rnerf/models.py:485-497) */
  const void* packed_coarse;   /* rnerf_nerfmlp_pack of coarse_mlp */
  const void* packed_fine;     /* rnerf_nerfmlp_pack of fine_mlp (NULL when num_fine == 0) */
  const float* bkgd_params;    /* float[RNERF_BKGDMLP_PARAMS] */
} rnerf_model;

/* Level outputs, struct-of-arrays in one buffer of 9*B floats (the 5-tuple of rnerf/models.py:359-361,532-535):
 * [0,3B) comp_rgb[B][3] | [3B,4B) distance[B] | [4B,5B) acc[B] | [5B,6B) trans[B] | [6B,9B) trans_rgb_bkgd[B][3]. */
#define RNERF_LEVEL_FLOATS 9

/* ---- device-resident jax.random keys (threefry2x32; pinned by tests/test_prng.py against values JAX publishes).
 * rnerf_rng_split3     : train_step's `rng, key_0, key_1 = random.split(rng, 3)` (train.py:74): rng_state uint32[2] is advanced in place,
 *                        keys4 uint32[4] receives (key_0, key_1).
 * rnerf_rng_forward    : the key chain of NerfModel.__call__: `key, rng_0 = split(rng_0)`; jitter = arange(0, N, P) (+ randint(key, [N_c],
 *                        0, P) when use_random_choice — also in eval, rnerf/models.py:240-242); `key, rng_1 = split(rng_1)` -> key_u, the key of
 *                        the stratified draws (rnerf/model_utils.py:345-354).  keys4 = (rng_0, rng_1); jitter int32[N_c]; key_u uint32[2].
 * rnerf_stratified_u_dev: rnerf_stratified_u with the key read from device memory. */
int rnerf_rng_split3(uint32_t* rng_state, uint32_t* keys4, void* stream);
int rnerf_rng_forward(const uint32_t* keys4, int32_t num_coarse, int32_t num_path, int32_t use_random_choice, int32_t* jitter, uint32_t* key_u,
                      void* stream);
int rnerf_stratified_u_dev(const uint32_t* key_dev, int32_t B, int32_t num_fine, float* u, void* stream);

/* ---- NerfModel.__call__ (rnerf/models.py:220-535; callers train.py:247, eval.py:97) for one batch of B rays: march -> background MLP on the
 * last coarse direction -> PE + coarse NerfMLP -> compositing [-> resampling -> PE + fine NerfMLP -> compositing (-> bd_cut pair)].
 * origins, viewdirs: float[B][3].  jitter: device int32[N_c] (rnerf_rng_forward, or any strictly increasing node indices).
 * u_fine (num_fine > 0): device float[N_f] shared by all rays (u_per_ray = 0; randomized=False: linspace(0, 1-eps, N_f)) or float[N_f][B].
 * out_coarse / out_fine: float[RNERF_LEVEL_FLOATS * B] (out_fine unused when num_fine == 0).
 * path_pd / path_dr (nullable, both or none): a path record float4[N][B] marched earlier for these rays (rnerf_march) — the march is
 * skipped; otherwise it runs here into the workspace.  workspace: rnerf_forward_workspace_bytes(m, B) bytes, 256-byte aligned.
 * max_workgroups: as rnerf_nerfmlp_forward. */
size_t rnerf_forward_workspace_bytes(const rnerf_model* m, int32_t B);
int rnerf_forward(const rnerf_model* m, const float* origins, const float* viewdirs, int32_t B, const int32_t* jitter, const float* u_fine,
                  int32_t u_per_ray, const float* path_pd, const float* path_dr, float* out_coarse, float* out_fine, void* workspace,
                  int32_t max_workgroups, void* stream);

/* ---- train_step.loss_fn + jax.value_and_grad (train.py:75-164) for the radiance stages: the training forward of every level, the loss
 * reductions, and the backward kernels down to the flat gradient.  theta: the flat fp32 parameter buffer [coarse_mlp | fine_mlp (if
 * num_fine > 0) | bkgd_mlp] (RNERF_NERFMLP_PARAMS, RNERF_NERFMLP_PARAMS, RNERF_BKGDMLP_PARAMS floats; m->packed_* / m->bkgd_params are
 * ignored: the operand streams are packed from theta inside the call).  grads: float[n_theta + 8]: d loss / d theta of THIS rank's rays
 * (before the mean over ranks, train.py:166; without the weight-decay term, which rnerf_adam_update adds) followed by the 8 stats scalars
 * of rnerf_train_stats.  pixels float[B][3]; env_dirs float[ps*ps][3] (bg_smooth_weight > 0).
 * keys4 (device uint32[4] = key_0, key_1 of rnerf_rng_split3) drives the jitter and the stratified draws; jitter_override / u_override
 * (nullable) inject them instead (parity tests).  path_pd / path_dr as in rnerf_forward. */
typedef struct rnerf_train_cfg {
  int32_t backward;            /* enum rnerf_backward */
  int32_t randomized;          /* FLAGS.randomized (rnerf/utils.py:131): stratified fine draws */
  int32_t use_random_choice;   /* rnerf/models.py:89 */
  int32_t bg_patch_size;       /* ps (0: no env-map smoothness term) */
  double bg_weight, bg_smooth_weight, annealed_alpha;     /* train.py:90-92,127-132 */
  double frozen_sq;            /* sum of squares / count of the variables outside theta (the frozen path_sampler): weight_l2, train.py:147-153 */
  int64_t frozen_count;
  void* aux_stream;            /* nullable: a second stream.  Everything of a step that depends on the parameters only — packing the operand streams of
                                  both directions, zeroing the gradient buffer, sum theta^2 — runs there beside the key kernels, the march and the
                                  background-MLP forward, and is joined inside the call before the first NerfMLP kernel.  At the other end of
                                  the step the env-map term, the background-MLP backward and the statistics run there, beside the last NerfMLP
                                  wgrad instead of behind it, joined before the call returns (the same kernels on the same operands: same bits).
                                  May be the same stream as grads_stream */
  void* grads_stream;          /* nullable: a stream the call orders behind the LAST NerfMLP wgrad (rnerf_fork at that point).  grads[0 .. NerfMLP
                                  segments) are final there: a caller with more than one rank starts their all-reduce (jax.lax.pmean, train.py:166 —
                                  95 % of the bytes) on this stream as soon as the call returns, and joins before rnerf_adam_update */
} rnerf_train_cfg;
/* The march of the NEXT batch (it reads neither the parameters nor anything of this step): when `next` is given, its rays are marched on
 * next->side_stream, forked from `stream` right before the last NerfMLP wgrad, so that the latency-bound march runs as co-resident waves
 * beside that HBM-paced kernel.  The caller joins (rnerf_join(stream, side_stream)) before it reads next->path_* — inside a captured graph:
 * before rnerf_graph_end. */
typedef struct rnerf_prefetch {
  const float* origins;        /* float[B][3] of the next batch */
  const float* viewdirs;
  float* path_pd;              /* float4[N][B] each: where the next batch's path record goes */
  float* path_dr;
  void* side_stream;
  /* Appended (RNERF_VERSION stays 4: the binding that fills this struct ships with the library).  Both null: every node is recorded.
   * Both given (flat models only): next_keys4 = the device uint32[4] (key_0, key_1) the NEXT step will pass as keys4; the call runs
   * rnerf_rng_forward on it on the side stream into sample_nodes (device int32[N_c]) and marches with rnerf_march_sparse.  The next step
   * must then read the path through exactly that array (its jitter_override). */
  const uint32_t* next_keys4;
  int32_t* sample_nodes;
} rnerf_prefetch;
size_t rnerf_train_workspace_bytes(const rnerf_model* m, const rnerf_train_cfg* c, int32_t B);
int rnerf_train_forward_backward(const rnerf_model* m, const rnerf_train_cfg* c, const float* theta, const float* origins, const float* viewdirs,
                                 const float* pixels, const float* env_dirs, int32_t B, const uint32_t* keys4, const int32_t* jitter_override,
                                 const float* u_override, int32_t u_per_ray, const float* path_pd, const float* path_dr, float* grads,
                                 void* workspace, int32_t max_workgroups, const rnerf_prefetch* next, void* stream);

/* ---- train.py:169-183 + optax.adam behind multi_transform (:312-317) on the flat buffers: weight-decay gradient 2 wd theta / n_all,
 * value clip, global-norm clip (over theta's gradient and the frozen variables' weight-decay gradient, frozen_params nullable),
 * Adam with bias correction and the reference's learning-rate schedule (rnerf/utils.py:490-528) evaluated on the device from the
 * device-resident step counter, which is incremented.  scratch: device float[RNERF_ADAM_SCRATCH_FLOATS] (no initial contents needed); after
 * the call scratch[3] holds the number of non-finite (inf / NaN) gradient entries the update met (0 in a healthy step: a forward row outside
 * f16's range, or a gradient chain beyond the 2^10 of headroom the f16 backward modes normalise every row to, makes that visible), counted
 * BEFORE the value clip (which would otherwise turn a NaN into +-grad_max_val).  skip_nonfinite != 0: an update that met such an entry
 * leaves theta, mu and nu untouched (the step counter still advances) — the reference's fp32 step would have been finite on that batch, so
 * the caller re-runs it in the range-safe arithmetic (precision BF16X3 + backward BF16; samplenerfro_amd.train does — by default two steps
 * later, from a pinned copy of scratch[3], without a per-step synchronisation) instead of writing NaN into every parameter. */
#define RNERF_ADAM_SCRATCH_FLOATS 3076
typedef struct rnerf_adam_cfg {
  double lr_init, lr_final, lr_delay_mult;
  int64_t max_steps, lr_delay_steps;
  double b1, b2, eps;
  double weight_decay_mult, grad_max_val, grad_max_norm;
  int64_t n_all;               /* number of variables weight_l2 averages over (theta + frozen) */
  double lr_override;          /* the learning rate of this update when use_lr_override != 0 (a replaced schedule, tests); 0.0 is honoured */
  int32_t use_lr_override;     /* 0: the reference's schedule (rnerf/utils.py:490-528) from the device-resident step counter */
  int32_t skip_nonfinite;      /* != 0: no update when a gradient entry is inf / NaN (see above) */
} rnerf_adam_cfg;
int rnerf_adam_update(const rnerf_adam_cfg* c, float* theta, float* mu, float* nu, float* grads, int64_t n_theta, const float* frozen_params,
                      int64_t n_frozen, int32_t* step_counter, float* scratch, void* stream);
/* The same update — the same bits in theta, mu, nu, grads, scratch[0..3] and the step counter — in two dependent launches instead of
 * three: the kernel that applies the update forms the scalars (learning rate, bias corrections, clip multiplier, non-finite count) in
 * every block from the per-block partials, with the additions rnerf_adam_update's one-workgroup launch performs.  (A configuration
 * without decay, clip and skip_nonfinite has no partials launch and keeps rnerf_adam_update's sequence.)  nonfinite_out (nullable): a
 * device-visible address, e.g. pinned host memory, that receives scratch[3] from the same launch — the word a host reads later without a
 * copy launch behind every step. */
int rnerf_adam_update_fused(const rnerf_adam_cfg* c, float* theta, float* mu, float* nu, float* grads, int64_t n_theta,
                            const float* frozen_params, int64_t n_frozen, int32_t* step_counter, float* scratch, float* nonfinite_out,
                            void* stream);

/* ---- one launch graph per step (hipGraph): begin capture on `stream`, issue any sequence of the calls above on it (and on streams forked
 * from it through rnerf_fork / rnerf_join), end -> an executable graph that replays the whole sequence with one launch. */
int rnerf_graph_begin(void* stream);
int rnerf_graph_end(void* stream, void** graph_exec);
int rnerf_graph_launch(void* graph_exec, void* stream);
int rnerf_graph_destroy(void* graph_exec);
/* side-stream helpers usable inside and outside capture: rnerf_fork makes `side` wait for everything issued on `main` so far;
 * rnerf_join makes `main` wait for everything issued on `side` so far (event pair owned by the library, per (main, side) call). */
int rnerf_fork(void* main_stream, void* side_stream);
int rnerf_join(void* main_stream, void* side_stream);

/* ---- Evaluation: SSIM.  Replaces utils.compute_ssim (rnerf/utils.py:404-471), called at train.py:449 and eval.py:187.
 * img0, img1: float[n][H][W][C] (channels last; each of the n leading images and each channel is an independent image); map (nullable):
 * float[n][H-fs+1][W-fs+1][C]; mean (nullable, not both null): float[n], the mean of each image's map.  The Gaussian window
 * (filter_size fs in [1, 31], filter_sigma > 0) is computed on the host in double by the reference's formula (:435-439) and rounded to
 * float once; c1 = (k1 max_val)^2, c2 = (k2 max_val)^2.  NaN propagates as in jnp.maximum / minimum / sign: a NaN pixel makes NaN every
 * map entry whose window covers it (in its channel) and that image's mean.  The mean is a fixed-order fp64 sum of per-tile partials in
 * `workspace` (rnerf_ssim_workspace_bytes, 8-byte aligned; unused when mean is null): the same inputs give the same bits on every run.
 * RNERF_ERR_ARG for fs outside [1, 31] or H < fs or W < fs, RNERF_ERR_UNSUPPORTED when (fs - 1) * C is so large that a tile's
 * input rows do not fit in LDS (C above about 580 at fs 11); the workspace query then returns 0. */
size_t rnerf_ssim_workspace_bytes(int64_t n, int32_t H, int32_t W, int32_t C, int32_t filter_size);
int rnerf_ssim(const float* img0, const float* img1, int64_t n, int32_t H, int32_t W, int32_t C, int32_t filter_size, double filter_sigma,
               double max_val, double k1, double k2, float* map, float* mean, void* workspace, void* stream);

/* ---- Evaluation: LDR-FLIP.  compute_ldrflip (metric/flip/flip_api.py:439-495) as metric/summary.py:72-78 calls it, on the device.
 * reference, test: float[n][H][W][3] (channels last, sRGB nominally in [0, 1]); map (nullable): float[n][H][W] (the filters replicate the
 * border); mean (nullable, not both null): float[n], the mean of each image's map.  pixels_per_degree (finite, > 0) sets the filters:
 * the spatial CSFs of generate_spatial_filter, radius r_s = ceil(3 sqrt(0.04 / (2 pi^2)) ppd), and the edge / point detectors of
 * feature_detection, radius r_f = ceil(3 * 0.5 * 0.082 ppd) <= r_s; their 1-D factors are computed on the host in double (the squared
 * distance rounded to float32 as there) and rounded to float once.  67.02 (compute_ldrflip's default) gives radii 10 and 9, 4.189
 * (summary.py) gives 1 and 1.  Both images go through one instruction sequence: where they agree on every pixel within r_s (border
 * replicated) of a pixel, the map there is exactly 0.  A NaN pixel makes NaN the map within r_s of it and that image's mean.
 * `workspace` (rnerf_flip_workspace_bytes, 8-byte aligned, always needed) holds one fp64 partial per 16 x 64 tile,
 * 8 n ceil(H / 16) ceil(W / 64) bytes, then 14 filtered planes, 56 n H W bytes; the mean is a fixed-order fp64 sum: the same inputs give
 * the same bits on every run.  RNERF_ERR_UNSUPPORTED when r_s > 15 (ppd above about 111) or when ppd is so small (below about 0.65) that
 * the detectors' off-centre weights vanish; the workspace query then returns 0. */
size_t rnerf_flip_workspace_bytes(int64_t n, int32_t H, int32_t W, double pixels_per_degree);
int rnerf_flip(const float* reference, const float* test, int64_t n, int32_t H, int32_t W, double pixels_per_degree, float* map,
               float* mean, void* workspace, void* stream);

/* ---- Capture scenes: visual-hull carving.  Replaces calib/make_visual_hull.py:107-146 (the voxel grid, the projection loop over the
 * views with project_2d :30-44, and the values of mesh.pkl), every step in float64 as there.  Appended; RNERF_VERSION stays 4.
 * masks: uint8[V][H][W], > 0 = object (cv2.imread(mask)[..., 0] > 0, :126,132); pv: double[V][12], the row-major 3 x 4 matrix
 * [cam_mat | 0] @ to_view_matrix(T) of each view (:40,92-93; formed on the host); g: the voxel grid, centres
 * linspace(0, 1, G)[i] * (nmax - nmin) + nmin (:112-120), count / out indexed [x][y][z], x slowest; g->layout is not read.
 * Per voxel and view: (a, b, c) = pv @ (x, y, z, 1), u = a / c, v = b / c, pixel (clip(round_half_even(v), 0, H - 1),
 * clip(round_half_even(u), 0, W - 1)) (:129-130); count = the number of views whose mask is set there.  No test of the sign of c, as in
 * the reference.  Where the reference is unspecified (c == 0, a NaN) the pixel clamps into the image: NaN -> 0, +-inf -> the edge.
 * Counts are integers kept in registers and stored once: no atomics, the same result on every run.
 * Limits (RNERF_ERR_ARG otherwise; checked before any device work): cubic grids, 2 <= G, G^3 < 2^31; 1 <= V < 2^31; H, W >= 1 and
 * H * W < 2^31.
 *   rnerf_visual_hull_workspace_bytes: 4 V H ceil(W / 32) — the masks packed to one bit per pixel (0 with a message for a bad size).
 *   rnerf_visual_hull_pack: fills `workspace` (4-byte aligned) from `masks`.
 *   rnerf_visual_hull_count: packs `masks` into `workspace` (masks == NULL: the workspace already holds the bits of these V views), then
 *     count = (accumulate ? count : 0) + views inside; accumulate (0 / 1) lets a host with hundreds of large masks upload them in chunks.
 *   rnerf_visual_hull_finalize: out = (count / total_views > threshold) ? ior_inside : ior_outside, the comparison in float64 (:136,141;
 *     the reference's values are 1.33 and 1.0). */
size_t rnerf_visual_hull_workspace_bytes(int64_t num_views, int32_t height, int32_t width);
int rnerf_visual_hull_pack(const uint8_t* masks, int64_t num_views, int32_t height, int32_t width, void* workspace, void* stream);
int rnerf_visual_hull_count(const uint8_t* masks, int64_t num_views, int32_t height, int32_t width, const double* pv, const rnerf_grid* g,
                            int32_t accumulate, int32_t* count, void* workspace, void* stream);
int rnerf_visual_hull_finalize(const int32_t* count, const rnerf_grid* g, int64_t total_views, double threshold, double ior_inside,
                               double ior_outside, float* out, void* stream);

/* ---- Preview meshes: marching cubes.  Replaces mcubes.marching_cubes at voxelize_mesh.py:122-135 (the voxelised grid's preview OBJ),
 * calib/make_visual_hull.py:148-157 (the carved hull's) and extract_mesh.py:232-268 (a trained field's density), on a grid that is already
 * on the device.  Appended; RNERF_VERSION stays 4.  PyMCubes' tie rule, vertex order and per-case triangulation are not reproduced; the
 * mesh is specified here instead, and is the same bytes on every run (no atomics).
 * field: float[dims[0]][dims[1]][dims[2]], axis 0 slowest.  A node is solid iff (double)f > iso, so NaN is empty and a plateau equal to iso
 * has no surface inside it.  Vertices: one per grid edge whose endpoints classify differently, owned by the edge's lower node, in node
 * order (axis 0 slowest) and within a node x-, y-, z-edge; double[V][3] in index units (sample i sits at coordinate i): the node's index
 * plus t = (iso - f1) / (f2 - f1) on the edge's axis, in float64 with every operation rounded, f1 the owning node's value; t = 0.5
 * where that is not within [0, 1] (non-finite endpoints), so every vertex is finite and on its edge.  Triangles: int32[F][3] vertex
 * indices, in cell order (a cell is named by its lowest node) and within a cell in the order of the case table; counter-clockwise seen
 * from the empty side, so a closed surface around higher values has a positive signed volume.  The table (tools/make_mc_tables.py)
 * cuts off each solid corner of an ambiguous face on its own; two cells that share a face agree there, so the surface of any field is
 * closed and consistently oriented except where it leaves the grid.
 * Limits (RNERF_ERR_ARG otherwise; checked before any device work): every dim >= 2 and 3 * dims[0] * dims[1] * dims[2] <= 2^31 - 1
 * (894^3 passes), iso finite, capacities >= 0.
 *   rnerf_marching_cubes_workspace_bytes: 8 ceil(N / 1024) + 4 N for N nodes (0 with a message for bad dims).
 *   rnerf_marching_cubes_count: two launches; fills `workspace` (8-byte aligned) and writes totals[0] = V, totals[1] = F (device, int64[2]).
 *   rnerf_marching_cubes_emit: with the same field, dims, iso and the workspace of _count; two launches.  Rows at or beyond a capacity
 *     are dropped and *overflow (device, zeroed by this call) is set to 1.  A capacity of 0 (its pointer may then be null) launches
 *     nothing of that kind and reports no overflow for it.  The vertex launch also writes every node's first vertex index into the
 *     workspace's per-node part, which the triangle launch reads: a call with verts_capacity 0 and faces_capacity > 0 is valid only
 *     after a call with verts_capacity > 0 on the same workspace.  What _count left in the workspace is only read, so _emit may be
 *     repeated.
 *   rnerf_marching_cubes_table: copies the case table the kernels use to tri_out, host int8[256][16]: up to five triangles of three edge
 *     ids per case, -1 padded.  Case bit x + 2y + 4z is set where corner (x, y, z) is solid; edge id = 4 axis + a + 2 b, (a, b) the base
 *     corner's coordinates on the two other axes, the lower axis first.  Needs no device. */
size_t rnerf_marching_cubes_workspace_bytes(const int32_t dims[3]);
int rnerf_marching_cubes_count(const float* field, const int32_t dims[3], double iso, void* workspace, int64_t* totals, void* stream);
int rnerf_marching_cubes_emit(const float* field, const int32_t dims[3], double iso, const void* workspace, double* verts,
                              int64_t verts_capacity, int32_t* faces, int64_t faces_capacity, int32_t* overflow, void* stream);
int rnerf_marching_cubes_table(int8_t* tri_out);

/* ---- Evaluation masks: the silhouette of a mesh.  Replaces the pyrender depth render of metric/render_mask.py:84-91 (an OpenGL context)
 * by a rasteriser over the camera model of rnerf_generate_rays.  Appended; RNERF_VERSION stays 4.
 * verts: double[V][3] world coordinates; faces: int32[F][3], every index in [0, V) — the caller's responsibility, they are not checked on
 * the device; camtoworld .. pixel_center: exactly the arguments of rnerf_generate_rays (opencv = 0: Blender model, cx = W/2, cy = H/2).
 * Pixel (row, col) is covered by a face iff the ray rnerf_generate_rays makes for it passes through the face, decided in float64 with every
 * operation rounded, as a 2-D test on the image plane:
 *   camera space   (xc, yc, zc) = Ri (p - t), each component ((Ri_j0 d0 + Ri_j1 d1) + Ri_j2 d2); t = camtoworld's translation widened from
 *                    float32, Ri = the inverse of its rotation widened from float32 (adjugate / determinant, formed on the host) — not
 *                    the transpose: a float32 rotation is orthogonal to about 1e-8 only, and the pixel's ray is t + lambda R cam;
 *   depth          = zc (OpenCV) or -zc (Blender): the distance along the view axis, what pyrender's depth buffer and Blender's Z pass
 *                    hold, not the ray parameter of the normalised viewdir;
 *   projection     X = (xc fx) / depth + cx,  Y = ((sy yc) fy) / depth + cy,  sy = -1 (Blender) or +1 (OpenCV),  w = 1 / depth,
 *                    fx, fy, cx, cy, pixel_center rounded to float32 first (as rnerf_generate_rays holds them);
 *   sample point   (x, y) = (col + pixel_center, row + pixel_center);
 *   orientation    area = (Bx - Ax)(Cy - Ay) - (By - Ay)(Cx - Ax); zero area covers nothing; sgn = +-1 its sign: either winding is
 *                    drawn (the Blender model mirrors the image plane), there is no back-face culling;
 *   edge function  of the edge P -> Q (AB, BC, CA): with (p, q) = (P, Q) if P <= Q lexicographically by (X, then Y), else (Q, P) and
 *                    s = sgn or -sgn accordingly, e = ((qx - px)(y - py) - (qy - py)(x - px)) s.  The two faces of a shared edge of a
 *                    consistently oriented mesh evaluate the same rounded expression with opposite signs;
 *   fill rule      inside the edge iff e > 0, or e == 0 and (dy > 0 or (dy == 0 and dx < 0)) with (dx, dy) = ((Qx - Px) sgn,
 *                    (Qy - Py) sgn): the top-left rule of rnerf_voxelize.  A sample on a shared edge belongs to exactly one of its two
 *                    faces, one on a vertex to exactly one face of the fan;
 *   depth          = (eab + ebc + eca) / ((ebc wA + eca wB) + eab wC) (perspective-correct: 1 / depth is linear in the weights), a hit
 *                    only where the first sum is > 0; kept iff znear < depth < zfar.
 * A face is tested at the pixels of the 16 x 16 pixel tiles (tile (i, j) = rows 16 i .., columns 16 j ..) that its pixel bounding box,
 * widened by one pixel on every side, meets — which matters only for what rounding could do far outside a degenerate face.
 * Outputs, none of which depends on the order of the face list or of any atomic: depth float[H][W] = float32 of the smallest kept depth,
 * 0 = nothing (render_mask.py:91 tests `depth != 0`); tri (nullable) int32[H][W] = the lowest face index among the hits that attain that
 * smallest float64 depth, -1 = nothing; hits (nullable) int32[H][W] = the number of kept hits (even everywhere for a closed mesh seen from
 * outside and inside [znear, zfar]).  The same inputs give the same bytes on every run, and a permuted face list the same depth and hits.
 * A face with a vertex at or behind the camera plane (depth <= 0, or a projection that is not finite) is not drawn and is counted in
 * *skipped (device int64[1], written by every call): there is no clipping, a camera inside the object is not a use of this.
 * Everything after the caller's upload runs on the device: projection, per-face tile range, per-tile lists (count, fixed-order scan, fill
 * through a cursor; a face that meets more than 4 tiles goes to one list that every tile walks, so the workspace depends on the sizes only).
 * num_faces == 0 is valid: the empty image, nothing that indexes the mesh is launched (verts, faces, workspace may be null).
 * RNERF_ERR_ARG before any device work: null camtoworld / depth / skipped, null verts / faces / workspace or num_verts == 0 with
 * num_faces > 0, num_verts outside [0, 2^31), num_faces outside [0, 2^29), H or W < 1, H * W >= 2^31, opencv not 0 / 1, fx or fy zero or
 * not finite, cx / cy / pixel_center not finite, a rotation without a finite inverse, not znear < zfar, verts / skipped not 8-byte or workspace not 16-byte aligned.
 *   rnerf_mesh_depth_workspace_bytes: 24 V + 36 F + 8 tiles + O(1), each part rounded up to 16 bytes (0 with a message for a bad size). */
size_t rnerf_mesh_depth_workspace_bytes(int64_t num_verts, int64_t num_faces, int32_t height, int32_t width);
int rnerf_mesh_depth(const double* verts, int64_t num_verts, const int32_t* faces, int64_t num_faces, const float* camtoworld /* HOST [3][4] */,
                     int32_t opencv, double fx, double fy, double cx, double cy, double pixel_center, int32_t height, int32_t width,
                     double znear, double zfar, float* depth, int32_t* tri, int32_t* hits, int64_t* skipped, void* workspace, void* stream);

/* ---- Evaluation masks: cv2.dilate(mask, np.ones((ky, kx)), iterations=1) with cv2's defaults (render_mask.py:92-93: 35 x 35) and
 * cv2.boundingRect of the result (metric/summary.py:202).  mask: uint8[H][W], > 0 = set; out: uint8[H][W], 255 where any pixel of the
 * ky x kx box centred on the pixel is set, else 0; pixels outside the image do not contribute.  A row pass into the workspace, then a
 * column pass.  bbox (nullable): device int32[4] = (x, y, w, h): the smallest set column and row of `out` and the extent to the largest,
 * both inclusive; (0, 0, 0, 0) when nothing is set.  It is reduced from one partial rectangle per 256 pixels in a fixed order (integer
 * minima and maxima).  RNERF_ERR_ARG before any device work: null mask / out / workspace, H or W < 1, H * W >= 2^31, ky or kx even or
 * < 1, out overlapping mask, workspace not 16-byte aligned.
 *   rnerf_mask_dilate_workspace_bytes: H W rounded up to 16, + 16 ceil(H W / 256) (0 with a message for a bad size). */
size_t rnerf_mask_dilate_workspace_bytes(int32_t height, int32_t width);
int rnerf_mask_dilate(const uint8_t* mask, int32_t height, int32_t width, int32_t ky, int32_t kx, uint8_t* out, int32_t* bbox,
                      void* workspace, void* stream);

/* ---- Evaluation: depth visualisations.  Replaces vis.visualize_suite as eval.py:175 calls it (rnerf/vis.py; JAX, jax.scipy's
 * convolve2d and matplotlib there).  Appended; RNERF_VERSION stays 4.  float32 per pixel in the order of the reference's formulas,
 * eps = 2^-23; every reduction is a fixed-order fold of per-block partials and the sort uses integer histograms: no float atomics, the
 * same inputs give the same bytes on every run.
 *
 * rnerf_vis_depth: visualize_depth (vis.py:45-111).  depth: float[H][W]; acc (nullable = all ones): float[H][W]; acc' = acc, 0 where
 * depth is NaN (:75).  near, far: NaN = automatic (the reference's `near or ...` also takes 0 as automatic; the caller maps it), else
 * rounded to float32.  Automatic bounds (:79-91): the pixels ordered by depth ascending, equal depths (-0 = +0) by pixel index, NaN last
 * (jnp.argsort); cum = the inclusive running sum of acc' in that order, total = its end; kept iff cum >= total * ignore_frac and
 * cum <= total * (1 - ignore_frac); near = the first kept depth - eps, far = the last kept depth + eps; both NaN when nothing is kept
 * (the reference raises there).  ignore_frac == 0 keeps every pixel and sorts nothing: one reduction, near = the minimum - eps (NaN when
 * every depth is NaN), far = the maximum + eps, or NaN if any depth is NaN.  ignore_frac > 0: a stable LSD radix sort of (key, pixel
 * index), four 8-bit passes of per-block histogram and scatter by in-block rank, then cum in fp64: (the sum of the earlier blocks' sums
 * + the earlier threads' sums) + the thread's own elements one by one, total = the sum of the blocks' sums, the two products and the
 * comparisons in fp64.  Nothing is ordered when both bounds are given.
 * curve (enum rnerf_vis_curve) is applied to depth, near and far (:94); the default of the reference is NEG_LOG.
 * modulus > 0 (:97-99): value = floored_mod(d, modulus) / modulus (jnp.mod: the sign of the divisor), colour = sinebow(value) (:23-26),
 * sin(pi x)^2 at 3/6 - v, 5/6 - v, 7/6 - v; NaN stays NaN.  modulus == 0 (:101-104): value = nan_to_num(clip((d - min(n, f)) / |f - n|,
 * 0, 1)), min propagating NaN, NaN -> 0; colour = matplotlib's `turbo`, a list of 256 colours (csrc/turbo_table.h), entry
 * min(int(value * 256), 255), not interpolated.  rgb = colour * acc' + (1 - acc') (:109).
 * Outputs, each nullable but not all: rgb float[H][W][3]; value float[H][W], the scalar before the colour map; range device float[2] =
 * (near, far) before the curve.
 *   rnerf_vis_depth_workspace_bytes: 4 KiB, and with ignore_frac > 0 another 16 H W + O(H W / 4) bytes (0 with a message for a bad size
 *   or ignore_frac).  The workspace (16-byte aligned) may be null when both bounds are given.
 *
 * rnerf_vis_normals: visualize_normals over depth_to_normals (vis.py:34-42, 114-132).  scaling: NaN = automatic (:116-122), over the
 * pixels whose depth is not NaN: sqrt(((var x + var y) / 2) / var depth), population variances of the column index, the row index and the
 * depth, each the fp64 sum of squared deviations from the fp64 mean (two passes of per-block partials), rounded to float32 once; equal
 * depths give +inf.  z = scaling * depth; dy = convolve2d(z, [-1, 0, 1]^T / 2 (x) [1, 2, 1] / 4, mode='same'), dx with the transposed
 * kernel: true convolutions, out[r][c] = sum over (p, q) of k[p][q] z[r + 1 - p][c + 1 - q] in that order from 0, zero outside the
 * image, all nine products formed — a NaN pixel makes dx and dy NaN in its 3 x 3 neighbourhood.  inv = 1 / sqrt((1 + dx^2) + dy^2),
 * normals = (dx inv, dy inv, inv).  rgb = isnan(normals) + nan_to_num((normals + 1) / 2), blended with the raw acc when acc is not null
 * (not zeroed at a NaN depth, as there).  Outputs, each nullable but not both: rgb float[H][W][3]; normals float[H][W][3], the vectors
 * before the colour step (what depth_to_normals returns, with scaling 1).
 *   rnerf_vis_normals_workspace_bytes: 16 KiB (0 with a message for a bad size); may be null when scaling is given.
 *
 * Both: RNERF_ERR_ARG before any device work for null required pointers, H or W < 1, H * W >= 2^31, ignore_frac outside [0, 0.5) or not
 * finite, modulus negative or not finite, an unknown curve, a workspace that is needed and null or not 16-byte aligned, an output that
 * overlaps an input or another output. */
enum rnerf_vis_curve {
  RNERF_VIS_CURVE_NEG_LOG = 0,      /* -log(x + eps) */
  RNERF_VIS_CURVE_IDENTITY = 1,
  RNERF_VIS_CURVE_RECIPROCAL = 2,   /* 1 / (x + eps) */
  RNERF_VIS_CURVE_LOG = 3           /* log(x + eps) */
};
size_t rnerf_vis_depth_workspace_bytes(int32_t height, int32_t width, double ignore_frac);
int rnerf_vis_depth(const float* depth, const float* acc, int32_t height, int32_t width, double near, double far, double ignore_frac,
                    int32_t curve, double modulus, float* rgb, float* value, float* range, void* workspace, void* stream);
size_t rnerf_vis_normals_workspace_bytes(int32_t height, int32_t width);
int rnerf_vis_normals(const float* depth, const float* acc, int32_t height, int32_t width, double scaling, float* rgb, float* normals,
                      void* workspace, void* stream);

/* ---- scene images (csrc/images.hip) ------------------------------------------------------------------------------------------------
 * rnerf_images_prepare: the pixel arithmetic of Blender / NSVF / OpenCV._load_renderings (rnerf/datasets.py:348-364, :394-414, :443-459)
 * on the decoded 8-bit views.  src: device uint8 [n][H][W][C], C = 3 (RGB) or 4 (RGBA, 4-byte aligned); dst: device float
 * [n][H / factor][W / factor][3].  Every operation is one correctly rounded float32 operation:
 *   factor 1: x = float(u) / 255.
 *   factor 2: x = float(u00 + u01 + u10 + u11) / 1020 per channel, alpha included: the mean of each 2 x 2 block from its exact integer
 *             sum (the reference averages four float32 u / 255 with cv2.INTER_AREA: at most 2^-22 away).  H, W even.
 *   white_bkgd (needs C == 4): out_c = x_c * x_a + (1 - x_a) on those values (:359-362); otherwise the first three channels.
 * One thread per output pixel, nothing allocated, no workspace.  RNERF_ERR_ARG before any device work for null pointers, C not 3 or 4,
 * factor not 1 or 2, odd H or W at factor 2, white_bkgd not 0 or 1 or set with C == 3, n, H or W < 1, 2^39 output pixels or more, a
 * misaligned pointer. */
int rnerf_images_prepare(const uint8_t* src, int64_t n, int32_t H, int32_t W, int32_t C, int32_t factor, int32_t white_bkgd, float* dst,
                         void* stream);

/* ---- error maps and the comparison sheet of metric/summary.py (csrc/metrics.hip, csrc/errmap.hip) --------------------------------------
 * Appended; RNERF_VERSION stays 4.  What summary.py writes per view besides its numbers: errmap/psnr_NNN.png, ssim_NNN.png, flip_NNN.png
 * and errmap/frame/frame_NNN.png.  The FLIP map is rnerf_flip's `map`, the LPIPS map (lpips_NNN.png, the third panel) rnerf_lpips' `map`, for a caller who has the weights.
 *
 * rnerf_errmap_mse: compute_psnr's map and mean squared error (summary.py:49-54).  reference, test: float[n][H][W][C]; map (nullable):
 * float[n][H][W], the mean over the channels of (reference - test)^2, every operation one rounded float32 operation, the channels added
 * in order; mean (nullable, not both null): float[n], the mean of the float32 squares of each image (summary.py:51) as a fixed-order fp64
 * sum of per-workgroup partials in `workspace` (rnerf_errmap_mse_workspace_bytes, 8-byte aligned; unused when mean is null): the same
 * inputs give the same bits on every run.  RNERF_ERR_ARG before any device work for null pointers, n, H, W or C < 1, more than 2^31
 * workgroups of 256 pixels, a map that overlaps an input. */
size_t rnerf_errmap_mse_workspace_bytes(int64_t n, int32_t H, int32_t W);
int rnerf_errmap_mse(const float* reference, const float* test, int64_t n, int32_t H, int32_t W, int32_t C, float* map, float* mean,
                     void* workspace, void* stream);

/* rnerf_ssim_summary: metric/ssim/ssim.py:45-133 (the pytorch-msssim formula) as summary.py:56-61,115 calls it — not rnerf_ssim's
 * formula.  img0, img1: float[n][H][W][C].  The Gaussian window (_fspecial_gauss_1d, :20-24; summary.py uses filter_size 11,
 * filter_sigma 1.5) is computed on the host in double and rounded to float once; "valid" convolution; C1 = (0.01 data_range)^2,
 * C2 = (0.03 data_range)^2 (summary.py: data_range 1);
 *   ssim = ((2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1)) * ((2 sigma12 + C2) / (sigma1^2 + sigma2^2 + C2)), nothing clamped.
 * map (nullable): float[n][H-fs+1][W-fs+1], the mean over the channels (size_average=True's ssim_map.mean(1)), unclipped — summary.py
 * clips it to [0, 1] before colouring, which rnerf_errmap_sheet's index does anyway; mean (nullable, not both null): float[n], the mean
 * of the unclipped per-channel maps, a fixed-order fp64 sum of per-tile partials: the same inputs give the same bits on every run.
 * `workspace` (rnerf_ssim_summary_workspace_bytes, 8-byte aligned, always needed): the partials, then the per-channel map
 * float[n][H-fs+1][W-fs+1][C], which a second launch averages over the channels.  The moments are those of rnerf_ssim (same tiles, same
 * shift before squaring), so sigma is closer to the exact value than ssim.py's float32 blur(x^2) - mu^2.  Argument checks and
 * RNERF_ERR_UNSUPPORTED as for rnerf_ssim; the workspace query then returns 0. */
size_t rnerf_ssim_summary_workspace_bytes(int64_t n, int32_t H, int32_t W, int32_t C, int32_t filter_size);
int rnerf_ssim_summary(const float* img0, const float* img1, int64_t n, int32_t H, int32_t W, int32_t C, int32_t filter_size,
                       double filter_sigma, double data_range, float* map, float* mean, void* workspace, void* stream);

/* rnerf_errmap_sheet: save_err and the merge of summary.py:40-45,223-240 as finished bytes, one launch.  reference, test: device
 * float[H][W][3]; maps, map_h, map_w: HOST arrays of K <= 4 device pointers float[map_h[k]][map_w[k]] with 1 <= map_h[k] <= H,
 * 1 <= map_w[k] <= W; out: device uint8[H][(2 + K)(W + 5)][3].  Columns: reference, 5 of 255, test, 5 of 255, then per map an H x W
 * panel — the coloured map in its top-left corner, 0 elsewhere — and 5 of 255.  An image value x becomes trunc(clip(255 x, 0, 255))
 * with the product in double (save_img on the float64 hstack); a map value v becomes the index i = trunc(clip(255 v, 0, 255)) with
 * the product in float32 (save_err) and then the bytes trunc(255 magma[i]) of csrc/magma_table.h (the PNG round trip of :233 is the
 * identity on bytes).  NaN, in an image or a map, gives byte or index 0: the reference's cast is undefined there.  The errmap PNGs are
 * slices of the sheet.  RNERF_ERR_ARG before any device work for null pointers, K outside [0, 4], H or W < 1, a map that is empty or
 * larger than the image, a sheet of 2^31 bytes or more, an `out` that overlaps an input. */
int rnerf_errmap_sheet(const float* reference, const float* test, int32_t H, int32_t W, int32_t K, const float* const* maps,
                       const int32_t* map_h, const int32_t* map_w, uint8_t* out, void* stream);

/* ---- LPIPS (csrc/lpips.hip).  Appended; RNERF_VERSION stays 4 -------------------------------------------------------------------------
 * rnerf_lpips: lpips.LPIPS(net='alex'), version 0.1, as metric/summary.py:63-68 calls it (model(ref, src, normalize=True)).  img0, img1:
 * device float[n][H][W][3] in [0, 1], H, W >= 31 (below it AlexNet's second pool is empty).  x = 2 img - 1, then (x - shift) / scale per
 * channel, shift = (-0.030, -0.088, -0.188), scale = (0.458, 0.448, 0.450); torchvision AlexNet `features` tapped after each ReLU: conv
 * 3->64 k 11 s 4 p 2 | MaxPool 3/2, conv 64->192 k 5 p 2 | MaxPool 3/2, conv 192->384 k 3 p 1 | conv 384->256 k 3 p 1 | conv 256->256
 * k 3 p 1 (cross-correlations, zero padding of the scaled input, floor pools).  Per tap l: f^ = f / (sqrt(sum_c f^2) + 1e-10),
 * d_l = sum_c lin_l[c] (f^0 - f^1)^2.
 * weights: device float[rnerf_lpips_weight_floats() = 2470848]: conv1.weight, conv1.bias, ..., conv5.weight, conv5.bias, lin0 .. lin4,
 * each in torch's own layout ([Cout][Cin][kh][kw]; lin_l: [C_l]).  The kernels read this buffer as it is; nothing is packed.
 * Outputs, each nullable but not all three:
 *   value      float[n]: sum over l = 0..4 of mean(d_l) (spatial=False), fixed-order fp64 sums of per-workgroup partials, rounded once;
 *   map        float[n][H][W]: sum over l = 0..4, in that order in float32, of d_l resized to H x W with torch's bilinear,
 *              align_corners=False (spatial=True), unclipped (summary.py:67 clips to [0, 1] before colouring);
 *   layer_maps float[n][P_0 + ... + P_4]: the five d_l of each pair back to back at their own resolutions P_l = h_l w_l,
 *              h_0 = (H - 7) / 4 + 1, h_1 = ((h_0 - 3) / 2 + 1), h_2 = h_3 = h_4 = (h_1 - 3) / 2 + 1 (integer divisions), w likewise.
 * The convolutions are implicit GEMMs in exact fp32 on the matrix cores (fp32 operands, fp32 accumulation, one k-ordered fused
 * multiply-add chain per output); both images of a pair go through them as one batch.  No atomics: the same inputs give the same
 * bytes, identical images give exactly 0, and swapping the images changes no byte.
 * `workspace`: rnerf_lpips_workspace_bytes(n, H, W) bytes, 8-byte aligned, always needed (activations, d_l, partials; about 61 MB for
 * one 800 x 800 pair).  The query returns 0 with the error set for n < 1, n > 65535, H or W < 31, or 2 n H W 3 >= 2^31.
 * RNERF_ERR_ARG before any device work for the same, null img0 / img1 / weights / workspace, all three outputs null, a workspace that
 * is not 8-byte aligned. */
size_t rnerf_lpips_weight_floats(void);
size_t rnerf_lpips_workspace_bytes(int64_t n, int32_t H, int32_t W);
int rnerf_lpips(const float* img0, const float* img1, int64_t n, int32_t H, int32_t W, const float* weights, float* map, float* value,
                float* layer_maps, void* workspace, void* stream);

/* ---- Connected components of a voxel grid (csrc/components.hip).  Appended; RNERF_VERSION stays 4 ------------------------------------
 * What the reference's README leaves to Blender ("remove the noisy components in the proxy geometry"): the floaters of a carved hull, of
 * a voxelised proxy mesh and of a trained density.  Grids are [X][Y][Z], z fastest, linear index x Y Z + y Z + z (the reference's flat
 * order); every dims[a] >= 1 and X Y Z <= 2^31 - 1, so that a label fits an int32.  All pointers are device pointers except dims.
 *   rnerf_components_label: solid uint8[X Y Z] (non-zero = solid); phase 1 labels the solid voxels, 0 the empty ones; connectivity 6
 *     (faces), 18 (faces and edges) or 26 (faces, edges and corners).  labels int32[X Y Z]: for a voxel of the labelled phase the smallest
 *     linear index in its component, -1 for every other voxel.  That is a pure function of the input: the same bytes on every run.
 *     Union-find with atomicMin hooking in three launches whatever the grid holds (8 x 8 x 64 tiles in LDS; tile faces, edges and corners
 *     with agent-scope atomics; flatten), nothing read back.  Every find / union loop is bounded by construction (parents only decrease)
 *     and has an iteration cap all the same; a kernel that reaches it sets word 0 of `workspace` (int32, zeroed by this call) and leaves:
 *     the labels are then not valid.  `workspace`: rnerf_components_workspace_bytes(dims) bytes, 4-byte aligned.
 *   rnerf_components_stats: from such labels, size int32[X Y Z] = the component's voxel count at its root index and 0 elsewhere, border
 *     uint8[X Y Z] = 1 at the root if a voxel of the component lies on one of the six faces of the grid and 0 elsewhere, counts int64[2] =
 *     {components, labelled voxels}.  All three are zeroed by the call.  Integer atomics after a per-wave reduction: exact.
 *   rnerf_components_apply: one launch over `grid` (dtype RNERF_COMPONENTS_U8 / _I32 / _F32, [X Y Z]): a voxel with labels[i] = r >= 0
 *     and keep[r] == 0 becomes drop_value; then one with fill_labels[i] = r >= 0 and fill[r] != 0 becomes fill_value; everything else is
 *     left as it is.  keep, fill: uint8[X Y Z] read at root indices.  Either pair (labels, keep) / (fill_labels, fill) may be null, not
 *     both.  The values are converted from double to the grid's type.
 * RNERF_ERR_ARG before any device work for null pointers, a dimension < 1, X Y Z >= 2^31 (the workspace query then returns 0 with the
 * message), a phase other than 0 / 1, a connectivity other than 6 / 18 / 26, an unknown dtype, a misaligned pointer. */
enum rnerf_components_dtype { RNERF_COMPONENTS_U8 = 0, RNERF_COMPONENTS_I32 = 1, RNERF_COMPONENTS_F32 = 2 };
size_t rnerf_components_workspace_bytes(const int32_t dims[3]);
int rnerf_components_label(const uint8_t* solid, const int32_t dims[3], int32_t phase, int32_t connectivity, int32_t* labels,
                           void* workspace, void* stream);
int rnerf_components_stats(const int32_t* labels, const int32_t dims[3], int32_t* size, uint8_t* border, int64_t* counts, void* stream);
int rnerf_components_apply(const int32_t* labels, const uint8_t* keep, double drop_value, const int32_t* fill_labels, const uint8_t* fill,
                           double fill_value, void* grid, int32_t dtype, const int32_t dims[3], void* stream);

/* ---- A/B comparison of two runs: metric/compare.py and metric/export.py's export_video (csrc/errmap.hip) ------------------------------
 * Appended; RNERF_VERSION stays 4.  The error maps of each run are those of the summary (rnerf_errmap_mse, rnerf_ssim_summary,
 * rnerf_lpips, rnerf_flip); these two calls turn them, and the runs' 8-bit images, into finished bytes.
 *
 * rnerf_compare_sheet: compare.py:216-236 as bytes.  maps_a, maps_b, map_h, map_w: HOST arrays of 1 <= K <= 4 device pointers
 * float[map_h[k]][map_w[k]] (the k-th error map of run A and of run B) with 1 <= map_h[k] <= H, 1 <= map_w[k] <= W; out: device
 * uint8[H][K (W + 5)][3].  Per element (:221-223), with d = |a - b| one rounded float32 subtraction:
 *   tie      d < float32(1e-3) (no float32 lies between 1e-3 and float32(1e-3): numpy's comparison with the Python float is the same set)
 *   A wins   not a tie and a <= b        B wins   not a tie and a > b        neither   a NaN on either side
 * inf - inf is NaN and so not a tie, and inf <= inf holds: two equal infinities are "A wins", as in numpy.  Bytes (:225-228 through
 * save_img, :40): A wins (239, 138, 98), tie (247, 247, 247), B wins (103, 169, 207), neither (0, 0, 0).  Each coloured map lies in the
 * top-left corner of an H x W panel of 255 (:230 np.ones — not rnerf_errmap_sheet's black panels), and 5 columns of 255 follow every
 * panel, the last included (:234).  compare.py's {name}_NNN.png are slices of this frame; the text labels of :232 are not drawn.
 * counts (nullable): device int64[K][4], 8-byte aligned, counts[k] = {A wins, tie, B wins, neither} over the map_h[k] x map_w[k]
 * elements of map k; the four add up to that element count.  The call clears it on `stream`; integer arithmetic only (per-wave
 * sums, LDS and global integer atomics), so the same inputs give the same numbers on every run.  One memset and one launch.
 * RNERF_ERR_ARG before any device work for null pointers, K outside [1, 4], H or W < 1, a map that is empty or larger than the image,
 * a frame of 2^31 bytes or more, a misaligned counts, an `out` or `counts` that overlaps a map or the other. */
int rnerf_compare_sheet(int32_t H, int32_t W, int32_t K, const float* const* maps_a, const float* const* maps_b, const int32_t* map_h,
                        const int32_t* map_w, uint8_t* out, int64_t* counts, void* stream);

/* rnerf_compare_strip: one frame of export.py:92-133 as bytes, one launch.  images: HOST array of 1 <= N <= 4 device uint8[H][W][3];
 * reference: device uint8[H][W][3]; out: device uint8[H][N (W + 5) + W][3].  Columns (:126-133): image 0, 5 of 255, ..., image N-1,
 * 5 of 255, the reference; no gap after the reference.  (rx, ry, rw, rh): the highlight rectangle of :93 (cv2.boundingRect's x, y, w,
 * h); rw == 0 or rh == 0: none.  With one, a byte v of an image outside it becomes (:102-108)
 *   trunc(clip(((v / 255.0) * 0.5 + 1.0 * 0.5) * 255.0, 0, 255))   in double
 * through a 256-entry table made on the host from that expression (not (v + 255) / 2: v = 73 gives 163, v = 105 gives 179); inside,
 * the same expression at weight 1 is the identity on every byte.  The reference is copied as it is: export.py fades only the
 * predictions.  The text labels of :111-115 are not drawn and the channel order is the caller's (the [..., ::-1] of :133 undoes
 * cv2.imread's BGR).  RNERF_ERR_ARG before any device work for null pointers, N outside [1, 4], H or W < 1, a rectangle that does not
 * lie inside the image, a strip of 2^31 bytes or more, an `out` that overlaps an input. */
int rnerf_compare_strip(const uint8_t* const* images, int32_t N, const uint8_t* reference, int32_t H, int32_t W, int32_t rx, int32_t ry,
                        int32_t rw, int32_t rh, uint8_t* out, void* stream);

/* ---- Bent-path diagnostics: refraction maps and path plots (csrc/paths.hip).  Appended; RNERF_VERSION stays 4 -------------------------
 * Records are float4 [num_nodes][B] as rnerf_march / rnerf_march_all write them: path_pd = (x, y, z, dist), path_dr = (dx, dy, dz, 0)
 * normalised, path_ior = (n, dn/dx, dn/dy, dn/dz).  All pointers are device pointers unless marked HOST.
 *
 * rnerf_path_summary: the per-pixel map eval.py:173,195 carries commented out (`pred_mask = any(|idx_grad| > 1e-3 along the path)`,
 * mask_{idx}.png) and what extract_mesh.py:178-223 reads off the pickled path of one pixel, for every ray at once.  Arithmetic is
 * individually rounded float32 unless stated, sqrt correctly rounded, sums of squares taken as (a a + b b) + c c.  Node k of ray r is
 * refracting when sqrt(sumsq(ior[k].yzw)) > (float)grad_eps: strict, and a NaN norm is not refracting (the reference's threshold is 1e-3,
 * eikonal_utils.py:35).  nodes int32[3][B]: [0] the count of refracting nodes, [1] the first such k, [2] the last, both -1 if none.
 * maps float[2][B]: [0] bend = sqrt(sumsq(dr[N-1].xyz - dr[0].xyz)) = 2 sin(theta / 2) of the total deflection theta; [1] optical =
 * (float) sum_{k=0}^{N-2} (double)(ior[k].x - 1.0f) (double)len_k with len_k = sqrt(sumsq(pd[k].xyz - pd[k+1].xyz)), the sum and the
 * products in float64, one term after the other in ascending k: the optical thickness of what the ray crossed beyond vacuum.  One launch,
 * one ray per lane, no atomics; every record of path_pd and path_ior is read once.  RNERF_ERR_ARG before any device work for null
 * pointers, num_nodes or B < 1, a NaN grad_eps, records not 16-byte aligned. */
int rnerf_path_summary(const float* path_pd, const float* path_dr, const float* path_ior, int32_t num_nodes, int32_t B, double grad_eps,
                       int32_t* nodes, float* maps, void* stream);

/* rnerf_path_plot: plt_utils.plot_path (called at extract_mesh.py:225; its four views :86) as finished bytes, without matplotlib: the
 * polylines of R selected rays in P orthographic panels.  rays int32[R]: ray indices into [0, B) (one outside is skipped); ray_rgb
 * uint8[R][3]; panels HOST double[P][2][4], 1 <= P <= 8; 1 <= size <= 8192; box HOST double[6] = (min x, y, z, max x, y, z), null: none;
 * floor_z: the plane of the shadow (:54), NaN: none; path_ior null: no markers; out uint8[P][size][size][3]; workspace:
 * rnerf_path_plot_workspace_bytes(P, size) bytes, 4-byte aligned.  The text, the axes and matplotlib's perspective are not reproduced.
 *   Pixel of a point: u = ((m00 x + m01 y) + m02 z) + m03 in float64 with every operation rounded, v from row 1 in the same way; column
 *   floor(u), row floor(v).  A point whose u or v is not finite or has |.| >= 2^30 cannot be drawn: its marker and the segments that
 *   touch it are skipped.
 *   Segment between the pixels (x0, y0) and (x0 + dx, y0 + dy): n = max(|dx|, |dy|); pixel i of n + 1 is (x0 + floor((2 i dx + n) / (2 n)),
 *   y0 + floor((2 i dy + n) / (2 n))) in int64, floor division; n = 0 is one pixel.  Only the i whose major coordinate lies inside the
 *   panel are visited, so a segment costs at most `size` iterations whatever its length.
 *   Drawn: the 12 box edges (edge e runs along axis e / 4 from min to max; bits 0 and 1 of e choose max on axes (e / 4 + 1) % 3 and
 *   (e / 4 + 2) % 3); per ray the segments node k -> k + 1, the same segments with z replaced by floor_z, and a 3 x 3 marker on every
 *   refracting node (the rule of rnerf_path_summary).  Every covered pixel inside the panel does atomicMax(key, layer << 28 | id), layers
 *   1 box, 2 shadow, 3 path, 4 marker, id = the slot j of the ray in `rays` or the edge number: an integer maximum does not depend on
 *   the order, so the bytes are the same on every run.  Colours: key 0 (255, 255, 255), box (255, 0, 0), shadow (139, 206, 151) (:55),
 *   path ray_rgb[j], marker (0, 0, 0).
 * One memset and two launches.  RNERF_ERR_ARG before any device work for null pointers, P or size out of range (the workspace query then
 * returns 0 with the message), R < 0 or >= 2^28, num_nodes or B < 1 with R > 0, a NaN grad_eps, misaligned pointers. */
size_t rnerf_path_plot_workspace_bytes(int32_t P, int32_t size);
int rnerf_path_plot(const float* path_pd, const float* path_ior, int32_t num_nodes, int32_t B, const int32_t* rays, const uint8_t* ray_rgb,
                    int32_t R, const double* panels /* HOST [P][2][4] */, int32_t P, int32_t size, const double* box /* HOST [6] */,
                    double floor_z, double grad_eps, void* workspace, uint8_t* out, void* stream);

/* ---- Ground-truth renderer for synthetic refractive scenes (csrc/scene.hip).  Appended; RNERF_VERSION stays 4 --------------------------
 * The image formation of the reference's `*_skydome-bkgd_no-partial-reflect_cycles` scenes, which is also what the model family represents:
 * an eikonal march through the IoR grid, an environment that depends on the last bent direction only, a grey medium in front of it.
 *
 * rnerf_scene_trace: the march of rnerf_march without path records.  table, g, origins [B][3], viewdirs [B][3], near, far, num_nodes as
 * there (both table layouts, the same size limits); every value of the recurrence is produced by the same individually rounded float32
 * operations in the same order, the step being (float)((far - near) / (num_nodes - 1)), wherever the grid coordinates (p - nmin) / ndelta
 * stay below 2^31 in magnitude (beyond, the cell fraction is taken from a saturated integer here and from floor(x) there).  Per ray:
 *   exit_dir float[B][4] = (safe_l2_normalize(d_{N-1}), 0): the bits rnerf_march writes into path_dr[N-1];
 *   counts int32[2][B]: [0] the number of nodes k in [0, N) with n(p_k) > (float)n_inside (strict; a NaN does not count), [1] the number of
 *   refracting nodes by the predicate of rnerf_path_summary, sqrt((a a + b b) + c c) > (float)grad_eps with the root correctly rounded
 *   and a NaN not refracting.
 * One launch; nothing of size N B is allocated or written.  RNERF_ERR_ARG before any device work for null pointers, B < 1, num_nodes < 2,
 * a NaN n_inside or grad_eps, a table or exit_dir that is not 16-byte aligned, a grid rnerf_march would refuse. */
int rnerf_scene_trace(const float* table, const rnerf_grid* g, const float* origins, const float* viewdirs, int32_t B, double near, double far,
                      int32_t num_nodes, double n_inside, double grad_eps, float* exit_dir, int32_t* counts, void* stream);

/* rnerf_scene_shade: the image from traced sub-pixel rays.  exit_dir float[(H K) (W K)][4] and counts int32[2][(H K) (W K)] are those of
 * the K times finer camera, row-major over (H K, W K); env float[6][E][E][3] is a cube map; albedo: HOST double[3], rounded to float.  One
 * thread per output pixel, its K K sub-samples taken in ascending (row, column) order of the fine image; every operation is an
 * individually rounded float32 operation unless stated, nothing is contracted.
 *   Cube map, for a direction d: m = max(|dx|, |dy|, |dz|), ties going to x before y before z; face 0..5 = +x, -x, +y, -y, +z, -z by the
 *   sign of that component; (s, t) = (a / m, b / m) with (a, b) = (y, z), (z, x), (x, y) on the x, y, z faces, no sign flips;
 *   u = ((s + 1) 0.5) E - 0.5 clamped to [0, E - 1], v from t likewise; i0 = floor, i1 = min(i0 + 1, E - 1), weight w = u - i0; bilinear as
 *   a (1 - w) + b w, along u in rows v0 and v1 and then along v, with env[face][v][u].  m == 0 and a direction with a NaN component give black, and so does
 *   a NaN face coordinate (inf / inf: two infinite components, which the rule above leaves without a texel); one infinite component
 *   looks up its face's centre.
 *   Sub-sample: T = (float)exp(((-sigma) step_len) (double)counts[0]) in float64 (exactly 1 when sigma == 0); colour = T env + (1 - T) albedo.
 *   Pixel: rgb float[H][W][3] = the sum of the K K colours in that order, from 0, times (float)(1.0 / (K K)) as one multiply; trans
 *   float[H][W] = the same mean of T; mask uint8[H][W] = 255 if any sub-sample has counts[1] > 0, else 0.
 * One launch, no atomics: the same bytes on every run.  RNERF_ERR_ARG before any device work for null pointers, H, W, K or E < 1,
 * H K W K beyond int32, an exit_dir that is not 16-byte aligned. */
int rnerf_scene_shade(const float* exit_dir, const int32_t* counts, int32_t H, int32_t W, int32_t K, const float* env, int32_t E, double step_len,
                      double sigma, const double* albedo /* HOST [3] */, float* rgb, float* trans, uint8_t* mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RNERF_H_ */
