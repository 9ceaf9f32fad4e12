/*
 * garmentnets_hip.h -- C ABI of libgarmentnets_hip.so (MI355X / gfx950).
 *
 * The reference (real-stanford/garmentnets) is pure Python and has no FFI of its own: its inference hot
 * path reaches native code only through third-party operator packages.  Each entry point below replaces
 * ONE such operator call site (cited as reference file:line) with a hand-written HIP kernel; the Python
 * host (garmentnets_amd/) binds them with ctypes and keeps the reference's module API on top
 * (INTEGRATION.md shows the binding a maintainer of the reference would add).
 *
 * Conventions
 *   - every function returns GN_OK (0) or a negative GN_E* code; gn_last_error() gives a thread-local message.
 *   - all pointers are DEVICE pointers into caller-owned memory unless the name ends in _host.
 *   - stream is a hipStream_t passed as void* (NULL = default stream); all work is stream-ordered, no
 *     allocation, no host synchronisation, no global mutable state (LUTs are immutable).
 *   - dense float tensors are fp32, row-major with an explicit leading dimension (ld*) in elements.  Exception: the two
 *     evaluation distances (gn_nearest_neighbor_f64_batch, gn_point_mesh_sqdist_batch) take and return fp64 tensors, and the two
 *     winding-number calls (gn_winding_number_batch, gn_winding_field_batch) take fp64 vertices; gn_distance_field_batch takes fp64
 *     vertices and returns fp64 squared distances; gn_cloth_simulate_batch is fp64 throughout.
 *   - volumes are CHANNEL-LAST: [B][D][H][W][C]  (the reference's NCDHW is a host-side view of this).
 *   - indices: point / vertex indices int32 on device (int64 only where the reference API exposes them).
 */
#ifndef GARMENTNETS_HIP_H
#define GARMENTNETS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GN_OK 0
#define GN_EINVAL (-1)   /* bad argument (shape / alignment / unsupported size) */
#define GN_ELAUNCH (-2)  /* HIP launch error */
#define GN_ECAP (-3)     /* caller-provided capacity too small (counts are still returned) */

const char *gn_last_error(void);
int gn_version(void);
/* name of the kernel variant the last gn_conv3d_gcr / gn_conv3d_gcr_split call of this thread launched (static string; ""
 * before the first call): measurement code labels its per-kernel timings with what really ran, not with a re-derived dispatch rule */
const char *gn_last_kernel(void);
/* number of CUs / XCDs the library sees on the current device (sanity: 256 / 8 on MI355X) */
int gn_device_info(int *num_cu, int *lds_bytes_per_cu);

/* ---------------------------------------------------------------------------------------------------------
 * Point-set operators (PointNet++).
 * ------------------------------------------------------------------------------------------------------- */

/* ptr[b] = first index i with batch[i] >= b, b = 0..B  (batch sorted ascending, int64).
 * replaces: PyG Batch bookkeeping used by every segmented op (components/pointnet2.py:26-29). */
int gn_segment_ptr(const int64_t *batch, int64_t n, int B, int32_t *ptr, void *stream);

/* Farthest point sampling.  replaces torch_cluster.fps -- components/pointnet2.py:26.
 * Per example b (points ptr[b]..ptr[b+1]) emits out_ptr[b+1]-out_ptr[b] indices (GLOBAL point index) starting
 * with local point start_idx[b] (start_idx == NULL: the example's first point = torch_cluster random_start=False; the
 * upstream default random_start=True is obtained by passing host-drawn random starts);
 * dist = (dx*dx+dy*dy)+dz*dz in fp32 without FMA; ties -> lowest index.
 * One workgroup per example (one wave per SIMD up to 24 points per lane), positions + running min-distance resident in registers / LDS. */
int gn_fps(const float *pos, const int32_t *ptr, const int32_t *out_ptr, const int32_t *start_idx, int B,
           int max_points_per_example, int32_t *out_idx, void *stream);

/* gn_fps for the CASCADE of components/pointnet2.py:26 (networks/pointnet2_nocs.py:139-141: sa2 samples the points sa1 selected).
 * gap_out    (NULL or [B] float): the smallest running maximum of the min-distance over this call's steps (3e38 if it took none).
 * nested_gap (NULL or [B] float): the gap_out of the EARLIER call whose output, in selection order, is this call's `pos` (caller's
 *            contract; start_idx must be NULL in both).  Farthest-point order is nested: with s_0..s_{m1-1} the earlier selection and
 *            D_k(i) = min_{j<k} d(i, s_j), position t of the new cloud holds E_k(t) = D_k(s_t) once positions 0..k-1 are chosen -- 0 for
 *            t < k, at most max_i D_k(i) = D_k(s_k) for t >= k -- so while that maximum is positive position k wins the arg-max and its
 *            lowest-index tie rule: an example with nested_gap[b] > 0 gets the indices ptr[b] + 0, 1, ..., m-1 without a single step,
 *            the others (duplicate-ridden clouds) are sampled as gn_fps samples them.  Same output as gn_fps, bit for bit, either way. */
int gn_fps_nested(const float *pos, const int32_t *ptr, const int32_t *out_ptr, const int32_t *start_idx, int B,
                  int max_points_per_example, int32_t *out_idx, float *gap_out, const float *nested_gap, void *stream);
/* gn_fps and gn_fps_nested take at most 36 864 points per example.  gn_fps_nested_ws takes any number: an example of more points keeps its
 * running distances in `ws`, one 16-byte record (x, y, z, d) per point, gn_fps_workspace_bytes(B, max_points_per_example) bytes (0 up to
 * 36 864 points: ws may then be NULL), 16-byte aligned.  Same arguments and the same output as gn_fps_nested otherwise, bit for bit. */
size_t gn_fps_workspace_bytes(int B, int max_points_per_example);
int gn_fps_nested_ws(const float *pos, const int32_t *ptr, const int32_t *out_ptr, const int32_t *start_idx, int B,
                     int max_points_per_example, int32_t *out_idx, float *gap_out, const float *nested_gap, void *ws, size_t ws_bytes,
                     void *stream);

/* Ball query.  replaces torch_cluster.radius(max_num_neighbors=K) -- components/pointnet2.py:28-29.
 * For every centre c (a point index centre_idx[c], example b): the first K points j of example b in ascending
 * index with d2(j,c) < r2 (strict).  nbr: [M][K] int32, -1 padded; cnt: [M].  One wavefront per centre
 * (ballot + popcount prefix keep the ascending order). */
int gn_ball_query(const float *pos, const int32_t *ptr, const int32_t *centre_idx, const int32_t *centre_ptr, int B,
                  int M, float r2, int K, int32_t *nbr, int32_t *cnt, void *stream);

/* Edge-feature gather for PointConv.  replaces PyG PointConv.message() gather -- components/pointnet2.py:31.
 * Row (c*(K+1)+s) of out = [x[j] (C floats), pos[j]-pos[centre_idx[c]] (3 floats)] for slot s of centre c, where
 * slots 0..K-1 are nbr[c][s] with the PointConv self-loop rule applied (a neighbour whose index equals the
 * centre ORDINAL c is dropped) and slot K is point c itself (add_self_loops on the bipartite graph);
 * self_loops=0 disables both.  Invalid slots are written as zeros and slot_src[c*(K+1)+s] = -1.
 * x may be NULL (C=0). */
int gn_sa_gather(const float *x, int ldx, int C, const float *pos, const int32_t *centre_idx, const int32_t *nbr,
                 int M, int K, int self_loops, float *out, int ldo, int32_t *slot_src, void *stream);
/* The same with the self-loop rule scoped by the caller: self_src[c] (int32 [M], or NULL = c: the call above) is the point that plays
 * "node c" on the source side -- dropped from centre c's neighbours, and the source of its added loop.  With self_src[c] = ptr[b] +
 * (c - centre_ptr[b]) (b = the centre's example) every example of a batch gets exactly what a batch of one would give it:
 * predict.py:62 asserts batch_size == 1, so that is the result the reference's pipeline produces for a garment. */
int gn_sa_gather_scoped(const float *x, int ldx, int C, const float *pos, const int32_t *centre_idx, const int32_t *nbr,
                        int M, int K, int self_loops, const int32_t *self_src, float *out, int ldo, int32_t *slot_src, void *stream);

/* out[c][ch] = max over valid slots s of in[c*S+s][ch].  replaces PointConv aggr='max' (scatter-max). */
int gn_segment_max(const float *in, int ldi, const int32_t *slot_src, int M, int S, int C, float *out, int ldo,
                   void *stream);

/* Set abstraction in ONE kernel: grouping gather -> 3-layer edge MLP (Linear -> ReLU -> eval-BatchNorm affine per layer, exact fp32
 * products on the matrix cores) -> segmented max, no edge tensor in HBM.  replaces PointConv(local_nn, aggr='max', add_self_loops)
 * on the radius graph -- components/pointnet2.py:20,31 (= gn_sa_gather + 3 x gn_linear + gn_segment_max, which remain for other MLP
 * shapes).  nbr/cnt: gn_ball_query's table (K <= 64, valid entries first); self_loops: PyG's bipartite quirk (centre i also receives
 * point i of the whole cloud; table entries equal to the centre's own index are dropped).  w1p/w2p/w3p/tab: garmentnets_amd.ops.
 * pack_sa_fused (A fragments [N/32][K blocks][4][64 lanes] x 16 B; per-unit bias | scale | shift in accumulator-register order).
 * Instantiated for the shipped edge MLPs [3+3,64,64,128] and [128+3,128,128,256] (gn_sa_fused_supported).  out [M][ldo]: max over
 * the centre's edges, 0 for a centre without edges. */
int gn_sa_fused_supported(int C, int N1, int N2, int N3);
int gn_sa_fused(const float *x, int ldx, int C, const float *pos, const int32_t *centre_idx, const int32_t *nbr, const int32_t *cnt,
                int M, int K, int self_loops, const float *w1p, const float *w2p, const float *w3p, const float *tab, int N1, int N2,
                int N3, float *out, int ldo, void *stream);
/* gn_sa_fused with the caller-scoped self-loop rule of gn_sa_gather_scoped (self_src: int32 [M] or NULL). */
int gn_sa_fused_scoped(const float *x, int ldx, int C, const float *pos, const int32_t *centre_idx, const int32_t *nbr, const int32_t *cnt,
                       int M, int K, int self_loops, const int32_t *self_src, const float *w1p, const float *w2p, const float *w3p,
                       const float *tab, int N1, int N2, int N3, float *out, int ldo, void *stream);
/* gn_sa_fused_scoped with the number of centres per workgroup chosen by the caller: group = 2, 4, 8, 16 or 32 forces that instantiation,
 * 0 runs the cost rule (what gn_sa_fused and gn_sa_fused_scoped do); anything else is GN_EINVAL before any launch.  Every group gives
 * the same bits (tests/test_gpu_pointnet2_forward_edges.py); the choice is a matter of speed alone.  x must be 16-byte aligned and ldx a
 * multiple of 4 when C >= 8 (the rows are read in 16-byte words). */
int gn_sa_fused_group(const float *x, int ldx, int C, const float *pos, const int32_t *centre_idx, const int32_t *nbr, const int32_t *cnt,
                      int M, int K, int self_loops, const int32_t *self_src, const float *w1p, const float *w2p, const float *w3p,
                      const float *tab, int N1, int N2, int N3, float *out, int ldo, void *stream, int group);
/* the group the cost rule takes for M centres of this edge MLP on the current device (GN_EINVAL: the MLP is not instantiated) */
int gn_sa_fused_auto_group(int C, int N1, int N2, int N3, int M);

/* out[b][ch] = max over rows ptr[b]..ptr[b+1].  replaces PyG global_max_pool -- components/pointnet2.py:49. */
int gn_global_max_pool(const float *in, int ldi, const int32_t *ptr, int B, int C, float *out, int ldo, void *stream);

/* k-NN inverse-squared-distance interpolation.  replaces PyG knn_interpolate -- components/pointnet2.py:72.
 * k <= 8; neighbours ordered by ascending (d2, index); w = 1/max(d2,1e-16); out = sum(w x)/sum(w). */
int gn_knn_interpolate(const float *xs, int ldx, const float *ps, const int32_t *ptr_s, const float *pq,
                       const int32_t *ptr_q, int B, int Nq, int C, int k, float *out, int ldo, void *stream);
/* The same for any k >= 1 (k <= 8: gn_knn_interpolate itself).  One pass per neighbour over the example's sources, in ascending (d2, index);
 * an example with fewer than k sources uses all of them. */
int gn_knn_interpolate_any(const float *xs, int ldx, const float *ps, const int32_t *ptr_s, const float *pq,
                           const int32_t *ptr_q, int B, int Nq, int C, int k, float *out, int ldo, void *stream);

/* Dense layer:  Y = bn( act( X W^T + bias ) ),  X [M][K] (ldx), W [N][K] (ldw), Y [M][N] (ldy).
 * relu != 0 applies ReLU; bn_scale/bn_shift (may be NULL) apply y*scale[n]+shift[n] AFTER the ReLU
 * (components/mlp.py:9-20: Linear -> ReLU -> BatchNorm1d in eval mode).  fp32 MFMA (v_mfma_f32_32x32x2_f32).
 * replaces torch.nn.Linear / ReLU / BatchNorm1d (ATen addmm + batch_norm) -- components/mlp.py:9-20,
 * networks/pointnet2_nocs.py:145-157, and the 1x1x1 final_conv components/unet3d.py:437,467. */
int gn_linear(const float *X, int ldx, const float *W, int ldw, const float *bias, const float *bn_scale,
              const float *bn_shift, int relu, int64_t M, int N, int K, float *Y, int ldy, void *stream);

/* NOCS head post-processing.  replaces argmax/softmax/gather + VirtualGrid.idxs_to_points --
 * networks/conv_implicit_wnf.py:220-231.  logits [N][bins*3] viewed as [N][bins][3]. */
int gn_nocs_head(const float *logits, int ldl, int64_t N, int bins, int64_t *bin_idx /*[N][3]*/, float *confidence /*[N][3]*/,
                 float *pred_nocs /*[N][3]*/, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Gridding (VolumeFeatureAggregator).
 * ------------------------------------------------------------------------------------------------------- */

/* Per-point aggregation features + target cell.  replaces VirtualGrid.get_points_grid_idxs / flatten_idxs /
 * idxs_to_points + torch.cat -- networks/conv_implicit_wnf.py:72-85, components/gridding.py:161-256.
 * out row = [feat (Cf), p - cell_corner (3), sim_pos (3), confidence (3)];  flat = ((b*G0+ix)*G1+iy)*G2+iz. */
int gn_grid_features(const float *feat, int ldf, int Cf, const float *nocs, const float *sim_pos, const float *conf,
                     const int64_t *batch, int64_t N, const float lower[3], const float upper[3], const int grid[3],
                     int include_point, int include_conf, float *out, int ldo, int32_t *flat_idx, void *stream);

/* Scatter point features into a zero-filled channel-last volume.  replaces torch_scatter.scatter(reduce) --
 * networks/conv_implicit_wnf.py:92-94.  reduce: 0 = max, 1 = mean, 2 = sum (torch_scatter's 'sum' and 'add'), 3 = min, 4 = mul.
 * vol [cells][C] is filled by this call (it does the memset); count_ws: [cells] int32 workspace, left zeroed.  Empty cells hold
 * the torch_scatter 2.0.8 value: 0 for max / mean / sum / min, 1 for mul.  Every reduction is deterministic (run-to-run
 * bit-identical): max / min by construction (atomicMax on an order-preserving encoding, bit-inverted for min), mean / sum
 * through order-independent fp64 partial sums, mul as a sequential fp32 product in ascending point index; the workspace `ws`
 * holds gn_grid_scatter_workspace_bytes(N, C, reduce) bytes (0 / NULL for max and min).  vol_is_zeroed != 0: the caller has already
 * zero-filled vol and count_ws (e.g. on a side stream, overlapped with the serial FPS kernels) and the memsets are skipped (mul
 * still writes its identity into every cell).  A NaN of either sign in any point of a cell makes that cell's channel NaN under every
 * reduction (torch.scatter_reduce's rule); the other cells are not affected. */
size_t gn_grid_scatter_workspace_bytes(int64_t N, int C, int reduce);
int gn_grid_scatter(const float *src, int lds, const int32_t *flat_idx, int64_t N, int C, int64_t cells, int reduce,
                    float *vol, int32_t *count_ws, void *ws, size_t ws_bytes, int vol_is_zeroed, void *stream);
/* gn_grid_scatter over channel-padded rows: channels [c_real, C) are pads (src holds zeros there), which mul's identity fill leaves at 0, so
 * the pads of every cell hold exact zeros under every reduction.  gn_grid_scatter = gn_grid_scatter_ex with c_real = C. */
int gn_grid_scatter_ex(const float *src, int lds, const int32_t *flat_idx, int64_t N, int C, int c_real, int64_t cells, int reduce,
                       float *vol, int32_t *count_ws, void *ws, size_t ws_bytes, int vol_is_zeroed, void *stream);

/* Output tiles (4 x 8 x 8 voxels, the tiling of gn_conv3d_gcr_split) of a 3x3x3 convolution over the scattered volume that can see an
 * occupied cell: flags [B][tiles_y * tiles_x * tiles_z] bytes (zeroed inside), index (ty * tiles_x + tx) * tiles_z + tz.  reach = 1 for the
 * convolution that reads the scattered volume, 2 for the one behind it (its input is non-constant within one voxel of the cells). */
int gn_grid_tile_flags(const int32_t *flat_idx, int64_t N, int B, int G0, int G1, int G2, int reach, unsigned char *flags, void *stream);

/* Per-(sample, channel) sum / sum of squares of a scattered volume computed from its OCCUPIED cells only (all other
 * cells are zero): the GroupNorm statistics of the first UNet layer without reading the (mostly empty) volume.
 * cells_per_sample = G0*G1*G2; sum/sumsq [B][C] fp64 (zeroed inside).  Must run after gn_grid_scatter on the same stream. */
int gn_grid_stats(const float *vol, const int32_t *flat_idx, int64_t N, int C, int64_t cells_per_sample, int B,
                  int32_t *count_ws, double *sum, double *sumsq, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * 3-D UNet (channel-last volumes [B][D][H][W][C]).
 * ------------------------------------------------------------------------------------------------------- */

/* Per-(sample, channel) sum and sum of squares over the V voxels, fp64 accumulators [B][C] (zeroed inside).
 * First half of nn.GroupNorm -- components/unet3d.py:66. */
int gn_channel_stats(const float *x, int B, int64_t V, int C, double *sum, double *sumsq, void *stream);

/* gn_channel_stats for any C % 4 == 0 (gn_channel_stats: C divides 256 or is a multiple of it).  One kernel serves both entries. */
int gn_channel_stats_any(const float *x, int B, int64_t V, int C, double *sum, double *sumsq, void *stream);

/* GroupNorm statistics -> per-(sample, channel) affine  y = x*a + d  for the concatenation of up to two
 * sources (src0: C0 channels, V0 voxels; src1: C1 channels, V1 voxels each replicated rep1 times = nearest
 * upsampling).  groups over C0+C1 channels, eps, biased variance (nn.GroupNorm).  a,d: [B][C0+C1].
 * act_inv_scale (NULL, or [B]): range normalisation for the split-operand convs -- a and d of sample b are multiplied by the power
 * of two that brings the largest per-channel rms of the normalised activations into [1, 2) and act_inv_scale[b] receives its
 * inverse (gn_conv3d_gcr_split undoes it exactly in its epilogue).  fp16 planes then cannot overflow for any checkpoint. */
int gn_groupnorm_affine(const double *sum0, const double *sq0, int C0, int64_t V0, const double *sum1, const double *sq1,
                        int C1, int64_t V1, int rep1, int B, int groups, float eps, const float *gamma,
                        const float *beta, float *a, float *d, float *act_inv_scale, void *stream);

/* gn_groupnorm_affine for any channel count (up to the 160 KB of LDS a workgroup has: 16 B per channel + 8 B per group) and for
 * channel-padded storage: source k holds Ck real channels in rows of Sk >= Ck stored ones (sum / sq [B][Sk]); the groups are formed over
 * the C0 + C1 real channels (gamma / beta [C0 + C1]); a, d [B][S0 + S1] in the stored layout with a = d = 0 on the pad channels.
 * gn_groupnorm_affine is this call with S0 == C0, S1 == C1 and its own limit of 1024 channels: one kernel serves both, and
 * padded storage gives the unpadded bits on the real channels. */
int gn_groupnorm_affine_map(const double *sum0, const double *sq0, int C0, int S0, int64_t V0, const double *sum1, const double *sq1,
                            int C1, int S1, int64_t V1, int rep1, int B, int groups, float eps, const float *gamma,
                            const float *beta, float *a, float *d, float *act_inv_scale, void *stream);

/* Fused GroupNorm-apply + Conv3d(3x3x3, pad 1, no bias) + ReLU, the 'gcr' SingleConv --
 * components/unet3d.py:53-66,19-76.  Input = channel concatenation [src0 (C0 ch, full res), src1 (C1 ch, HALF
 * res, nearest-upsampled on the fly)] (torch.cat((skip, up(x))) of components/unet3d.py:291,330); src1 may be
 * NULL.  Zero padding is applied AFTER the affine (as nn.Conv3d pads the normalised tensor).
 * wp: weights repacked [27 taps][Cin/16 slices][Cout][16] (tap = (kd*3+kh)*3+kw, channel = slice*16 + k).
 * out_sum / out_sumsq (both NULL or both [B][Cout] fp64, zeroed inside): per-(sample, channel) sum and sum of squares
 * of the OUTPUT, i.e. the GroupNorm statistics of the next layer, produced by the epilogue.
 * LDS-tiled implicit GEMM on fp32 MFMA. */
int gn_conv3d_gcr(const float *src0, int C0, const float *src1, int C1, const float *a, const float *d,
                  const float *wp, int B, int D, int H, int W, int Cout, int relu, float *out, double *out_sum,
                  double *out_sumsq, void *stream);

/* Split-operand variant of gn_conv3d_gcr on the 16-bit matrix cores (GN_SPLIT_F16X2 is what garmentnets_amd uses by default;
 * gn_conv3d_gcr is the plain fp32-MFMA kernel): identical contract, but the
 * fp32 operands are decomposed into low-precision planes (x = x1 + x2 [+ x3], exact residual chain) and multiplied on the
 * 16-bit matrix cores with fp32 accumulation:
 *   GN_SPLIT_BF16X3: 3 bf16 planes, 6 partial products, dropped terms <= 2^-24 relative (fp32-class products)
 *   GN_SPLIT_F16X2 : 2 fp16 planes, 3 partial products, operand residual and dropped term <= 2^-22 relative for operands within
 *                    2^3 of their scale (below: absolute, 2^-25 of the scale).  Scales: one power of two per OUTPUT CHANNEL for the
 *                    weights (row maximum in [1, 2)) and one per SAMPLE for the activations (gn_groupnorm_affine act_inv_scale)
 *   GN_SPLIT_BF16X2: 2 bf16 planes, 3 partial products, 2^-16 relative (fast preview quality)
 * wp_planes: weight pack in MFMA-fragment order [Cin/16][27 taps][Cout/32][planes][64 lanes] x 16 B + eight zero steps
 * (garmentnets_amd.ops.pack_conv_weight_split); out_scale [Cout]: the exact powers of two that undo the pack's per-output-channel
 * weight scales (all 1 for bf16); act_inv_scale: NULL or [B] from gn_groupnorm_affine. */
#define GN_SPLIT_BF16X2 2
#define GN_SPLIT_BF16X3 3
#define GN_SPLIT_F16X2 4
/* Occupancy-aware launch (the layer whose input is gn_grid_scatter's volume, > 99 % empty for 6000 points in 128^3 cells):
 * tile_active (NULL, or [B][tiles] bytes from gn_grid_tile_flags) marks the 4 x 8 x 8 output tiles whose halo holds an occupied cell;
 * every other tile's outputs are border-class constants kconst [B][(2r+1)^3][Cout], r = kreach (class (cz*n + cy)*n + cx with, per
 * axis, c = z for z < r, 2r - (D-1-z) for z >= D-r, r otherwise; the FINISHED values a dense launch produces there -- garmentnets_amd
 * takes them from dense launches of the same layers over a 5 x 5 x 5 all-zero volume with the same affines) and are stored without
 * touching the matrix cores.  kreach = 1: the layer fed by the scattered volume; 2: the layer behind it.  The output is bit-identical
 * to the dense launch.  Two-plane modes only.  The call builds a compact, ascending list of the active tiles in occ_ws
 * (gn_conv3d_occupancy_workspace_bytes(B, D, H, W) bytes; required with tile_active), fills the inactive tiles (constants + their share of
 * out_sum / out_sumsq) with an HBM-bound kernel and runs the convolution kernel over the listed tiles only. */
size_t gn_conv3d_occupancy_workspace_bytes(int B, int D, int H, int W);
/* `partial` (NULL, or [B][D/2][H/2][W/2][8][Cout] from gn_upconv_partial): the polyphase form of a layer whose second source is
 * nearest-upsampled -- this launch then covers the full-resolution source alone (src1 NULL) and its epilogue adds
 * partial[b][z>>1][y>>1][x>>1][(z&1)*4 + (y&1)*2 + (x&1)][n] before the ReLU. */
int gn_conv3d_gcr_split(const float *src0, int C0, const float *src1, int C1, const float *a, const float *d,
                        const void *wp_planes, int mode, const float *out_scale, const float *act_inv_scale, int B, int D, int H, int W,
                        int Cout, int relu, float *out, double *out_sum, double *out_sumsq, const unsigned char *tile_active,
                        const float *kconst, int kreach, const float *partial, void *occ_ws, size_t occ_ws_bytes, void *stream);

/* The GroupNorm affine folded into PER-SAMPLE weights (csrc/conv_prep.hip) -- for a 'gcr' layer (components/unet3d.py:66-76) whose input
 * is AT REST almost everywhere: the scattered volume of networks/conv_implicit_wnf.py:92-94 (zero outside the occupied cells) and the
 * layer behind it (one value per channel away from them).  conv(a x + d) is linear, so with c = the rest value (coff [B][Cin]; NULL =
 * zeros) and s a per-(sample, channel) power of two
 *     conv_w(a x + d)[n] = sum_taps sum_ch (w a / s) ((x - c) s)  +  sum_{taps inside the volume} sum_ch w (a c + d):
 * the operand (x - c) s is EXACTLY ZERO wherever x == c, the shift becomes the per-(sample, border class, output channel) constant kbias.
 * Same MACs through the same kernels; the matrix cores see mostly zeros and draw less power, which under the socket power cap is clock
 * (DESIGN.md 5.1).  gn_conv_affine_pack prepares, from the raw Conv3d weight w [Cout][Cin][3][3][3], the GroupNorm affine a, d [B][Cin]
 * (gn_groupnorm_affine without the sample scale) and the input's statistics sum / sumsq [B][Cin] over V voxels:
 *     stage_a, stage_d [B][Cin]  the staging affine (s, -c s), s = 2^k with rms(x - c) s in [1, 2)
 *     pack                       [B] fp16x2 weight sets (w a / s, row-scaled to [1, 2)) in the fragment order of gn_conv3d_gcr_split,
 *                                gn_conv_affine_pack_bytes(B, Cin, Cout) bytes
 *     out_scale [B][Cout]        exact powers of two undoing the row scales
 *     kbias [B][64][Cout]        class = (mz * 4 + my) * 4 + mx, m = (voxel has a previous neighbour on the axis) | (a next one) << 1
 * ws: gn_conv_affine_pack_workspace_bytes(B, Cin, Cout) bytes (both entries), on 8 bytes.  gn_conv3d_gcr_split_persample runs the layer from them (GN_SPLIT_F16X2 arithmetic, one source;
 * tile_active / kconst / kreach / partial / occ_ws as gn_conv3d_gcr_split). */
size_t gn_conv_affine_pack_bytes(int B, int Cin, int Cout);
size_t gn_conv_affine_pack_workspace_bytes(int B, int Cin, int Cout);
int gn_conv_affine_pack(const float *w, int Cin, int Cout, const float *a, const float *d, const double *sum, const double *sumsq, int64_t V,
                        const float *coff, int B, void *pack, size_t pack_bytes, float *stage_a, float *stage_d, float *out_scale,
                        float *kbias, void *ws, size_t ws_bytes, void *stream);
int gn_conv3d_gcr_split_persample(const float *src, int Cin, const float *stage_a, const float *stage_d, const void *pack,
                                  const float *out_scale, const float *kbias, int B, int D, int H, int W, int Cout, int relu, float *out,
                                  double *out_sum, double *out_sumsq, const unsigned char *tile_active, const float *kconst, int kreach,
                                  const float *partial, void *occ_ws, size_t occ_ws_bytes, void *stream);

/* Winograd F(2,3) along x for the 128-wide 'gcr' convolution (csrc/unet_wino.hip; components/unet3d.py:53-76, the shape it exists for:
 * the first encoder convolution 128 -> 128 at full resolution, components/unet3d.py:127-133): per output pair (x, x+1) and (kd, kh, channel)
 * FOUR products m0 = (d0 - d2) g0, m1 = (d1 + d2)(g0 + g1 + g2)/2, m2 = (d2 - d1)(g0 - g1 + g2)/2, m3 = (d1 - d3) g2 instead of six --
 * 36 instead of 54 matrix-core tap products per output pair, GN_SPLIT_F16X2 arithmetic on the transformed operands (input transform in
 * fp32 before the plane split, weight transform in fp64 on the pack side, output transform in fp32).  Exactly-zero operands stay exactly zero.
 * ONE entry for both operand forms:
 *   kbias == NULL: the literal form.  a, d [B][Cin] = gn_groupnorm_affine (with its act_inv_scale [B], or NULL); pack = the transformed
 *                  static weights [Cin/16][36 steps = (j * 3 + kd) * 3 + kh][Cout/32][2 planes][64 lanes] x 16 B + six zero steps
 *                  (garmentnets_amd.ops.pack_conv_weight_split_wino); out_scale [Cout].
 *   kbias != NULL: the affine-in-weights form -- a, d, pack, out_scale [B][Cout], kbias [B][64][Cout] from gn_conv_affine_pack_wino
 *                  (same contract as gn_conv_affine_pack, 36 steps per slice: gn_conv_affine_pack_wino_bytes); act_inv_scale NULL.
 * Requirements (GN_EINVAL otherwise): one source, Cin % 16 == 0, D*H*W <= 2^27, D*H*W*Cin*4 < 2^32 and
 *   Cout % 128 == 0 (csrc/unet_wino.hip: 4 x 8 x 8 tiles x 128 channels): Cin <= 256, D % 4 == H % 8 == W % 8 == 0;
 *   any other Cout % 32 == 0 (csrc/unet_wino32.hip, round 6: one kernel, 8 x 8 x 8 tiles x one 32-wide column block, four waves multiplying and four
 *   staging -- the encoder's second convolution 128 -> 32 at full resolution, components/unet3d.py:127-144, and the last decoder's convolutions,
 *   :291,330): Cin <= 128, D % 8 == H % 8 == W % 8 == 0.
 * tile_active / kconst / kreach / occ_ws as gn_conv3d_gcr_split (tile granularity of the occupancy-aware list: the kernel's own).
 * gn_conv3d_gcr_split_wino_partial: the same layer with the polyphase partial of gn_upconv_partial added before the ReLU (Cout % 128 != 0 only; dense). */
size_t gn_conv_affine_pack_wino_bytes(int B, int Cin, int Cout);
int gn_conv_affine_pack_wino(const float *w, int Cin, int Cout, const float *a, const float *d, const double *sum, const double *sumsq, int64_t V,
                             const float *coff, int B, void *pack, size_t pack_bytes, float *stage_a, float *stage_d, float *out_scale,
                             float *kbias, void *ws, size_t ws_bytes, void *stream);
int gn_conv3d_gcr_split_wino(const float *src, int Cin, const float *a, const float *d, const void *pack, const float *out_scale,
                             const float *act_inv_scale, const float *kbias, int B, int D, int H, int W, int Cout, int relu, float *out,
                             double *out_sum, double *out_sumsq, const unsigned char *tile_active, const float *kconst, int kreach,
                             void *occ_ws, size_t occ_ws_bytes, void *stream);
int gn_conv3d_gcr_split_wino_partial(const float *src, int Cin, const float *a, const float *d, const void *pack, const float *out_scale,
                                     const float *act_inv_scale, const float *kbias, int B, int D, int H, int W, int Cout, int relu, float *out,
                                     double *out_sum, double *out_sumsq, const float *partial, void *stream);

/* The nearest-upsampled source of a decoder convolution in polyphase form (torch.cat((skip, interpolate(x, 'nearest'))) -> Conv3d,
 * components/unet3d.py:291,330): every fine output voxel (2i+pz, 2j+py, 2k+px) sees only a 2 x 2 x 2 block of coarse voxels, so the 27
 * fine taps merge into 8 coarse taps per output parity class (sums of weights, host side, fp64) -- 8/27 of the MACs of those channels,
 * and the coarse halo is staged once for all classes instead of once per fine voxel.  src1 [B][Dc][Hc][Wc][C1]; a, d [B][C1]: the
 * GroupNorm affine of THESE channels (contiguous slices of gn_groupnorm_affine's result); wp: merged weights in fragment order
 * [C1/16][8 taps][8 classes][Cout/32][2 planes][64 lanes] x 16 B with out_scale [8 * Cout] (garmentnets_amd.ops.pack_upconv_weight);
 * partial [B][Dc][Hc][Wc][8 * Cout] in true units, no activation.  Arithmetic: the two-plane split of gn_conv3d_gcr_split. */
int gn_upconv_partial(const float *src1, int C1, const float *a, const float *d, const void *wp, int mode, const float *out_scale,
                      const float *act_inv_scale, int B, int Dc, int Hc, int Wc, int Cout, float *partial, void *stream);

/* The STATIC split-operand weight packs built on the device (csrc/weight_pack.hip) from the raw contiguous Conv3d weight w [Cout][Cin][3][3][3]
 * (components/unet3d.py:53-56): what garmentnets_amd.ops.pack_conv_weight_split / pack_conv_weight_split_wino / polyphase_weights +
 * pack_upconv_weight build on the host, without a host round trip -- a training step rebuilds every pack after each optimiser step.  No
 * intermediate tensor in device memory, nothing read back; each entry writes the whole pack (zero steps included) and out_scale.
 *   gn_weight_pack_split       input channels [c_lo, c_lo + c_n) (c_lo = 0, c_n = Cin: the plain layer; [0, C0): the full-resolution part of a
 *                              polyphase layer) -> [c_n/16][27 taps][Cout/32][planes][h 2][r 32][8] x 16 bit + eight zero steps (lane 32 h + r
 *                              holds channels 8h..8h+7 of output 32 blk + r), the pack of gn_conv3d_gcr_split; planes by the residual chain
 *                              p = rn(r), r -= float(p), round to nearest even; mode GN_SPLIT_F16X2 / GN_SPLIT_BF16X2 / GN_SPLIT_BF16X3;
 *                              out_scale [Cout] (all 1 for the bf16 modes)
 *   gn_weight_pack_split_wino  the same range -> [c_n/16][36 steps = (j * 3 + kd) * 3 + kh][Cout/32][2 planes][h][r][8] + six zero steps, the
 *                              literal-form pack of gn_conv3d_gcr_split_wino: the F(2,3) positions (g0, (g0 + g1 + g2)/2, (g0 - g1 + g2)/2, g2)
 *                              in fp64, row scale over the TRANSFORMED row, one rounding to fp32 after scaling, two fp16 planes; out_scale [Cout]
 *   gn_weight_pack_upconv      input channels [c0, Cin) = C1 -> [C1/16][tap 4 iz + 2 iy + ix][class 4 pz + 2 py + px][Cout/32][2 planes][h][r][8],
 *                              the pack of gn_upconv_partial: the 27 fine taps merged in fp64 into the 2 x 2 x 2 coarse taps of each parity
 *                              class, each merged tap rounded to fp32 once; one scale per (class, output): out_scale [8 * Cout];
 *                              mode GN_SPLIT_F16X2 / GN_SPLIT_BF16X2
 * Row scale (fp16 planes): 2^k with k from the exponent field of the row maximum m, so that m 2^k lies in [1, 2); 1 for a zero or
 * non-finite maximum; k clamped to +-100.  The host builders document the same rule but compute exp2(-floor(log2(m))), which rounds up for
 * m a few ulps below a power of two (fp32: two ulps below 2^-4, four below 2^-10): there the host leaves the maximum in [0.5, 1) and its
 * out_scale is twice this one.  Both decompositions are exact; away from those rows the packs agree bit for bit.
 * pack: 16-byte aligned, at least gn_weight_pack_*_bytes (0: widths the entries refuse).  GN_EINVAL: c_n % 16 != 0, Cout % 32 != 0, a
 * channel range outside the weight, an unknown mode. */
size_t gn_weight_pack_split_bytes(int c_n, int Cout, int mode);
size_t gn_weight_pack_split_wino_bytes(int c_n, int Cout);
size_t gn_weight_pack_upconv_bytes(int C1, int Cout);
int gn_weight_pack_split(const float *w, int Cout, int Cin, int c_lo, int c_n, int mode, void *pack, size_t pack_bytes, float *out_scale,
                         void *stream);
int gn_weight_pack_split_wino(const float *w, int Cout, int Cin, int c_lo, int c_n, void *pack, size_t pack_bytes, float *out_scale,
                              void *stream);
int gn_weight_pack_upconv(const float *w, int Cout, int Cin, int c0, int mode, void *pack, size_t pack_bytes, float *out_scale, void *stream);

/* The pieces of create_conv's layer orders other than 'gcr'(components/unet3d.py:19-73: 'cr', 'crg', 'cl', 'ce', 'bcr', ...) that the fused conv
 * kernels do not cover -- a learnable conv bias, LeakyReLU(0.1) / ELU, a normalisation BEHIND the non-linearity:
 * y = act(x * a[b][c] + d[b][c] + bias[c]) over channel-last [B][V][C] (C % 4 == 0); a / d ([B][C], together) and bias ([C]) may be NULL;
 * act: 0 none, 1 ReLU, 2 LeakyReLU(0.1), 3 ELU(alpha 1).  In place when out == x. */
int gn_affine_act(const float *x, int B, int64_t V, int C, const float *a, const float *d, const float *bias, int act, float *out, void *stream);

/* MaxPool3d(2) -- components/unet3d.py:222.  in [B][D][H][W][C] -> out [B][D/2][H/2][W/2][C].
 * out_sum / out_sumsq: optional statistics of the pooled output (as gn_conv3d_gcr). */
int gn_maxpool3d_2(const float *in, int B, int D, int H, int W, int C, float *out, double *out_sum, double *out_sumsq,
                   void *stream);
/* ---------------------------------------------------------------------------------------------------------
 * Implicit decoder.
 * ------------------------------------------------------------------------------------------------------- */

/* Trilinear feature sampling.  replaces F.grid_sample(bilinear, border, align_corners=True) on a 5-D input --
 * networks/conv_implicit_wnf.py:135-145 (including its axis convention: query x -> LAST volume axis).
 * vol: one sample [D][H][W][C].  If query == NULL the queries are the lattice of predict.py:145-147:
 * q[i][j][k] = (i,j,k) * (1/(Q-1)), rows m0..m0+M of the flattened (Q,Q,Q) lattice.
 * vol is PACKED fp32 (no strides).  Alignment: channels are moved in 16-byte accesses when C is 4, 8, 16, 32, 64 or 128 and ldo % 4 == 0, and whenever the lattice
 * brick kernel serves the call (query == NULL, C % 32 == 0, ldo % 4 == 0, whole i-slabs, Q >= D, H, W); in 8-byte accesses for every other even C (ldo must be even);
 * one float at a time for odd C.  vol and out must be aligned to the access size: GN_EINVAL otherwise, before any launch.
 * A NaN query component samples source index 0 (fmax's rule; ATen's std::max chain gives size - 1).  Results are ATen's grid_sampler_3d bits, with one exception in
 * the brick kernel: where the lower cell corner (x0, y0, z0) holds +-inf and the query lies on an upper face of the volume it returns NaN, not +-inf. */
int gn_trilinear_sample(const float *vol, int D, int H, int W, int C, const float *query, int Q, int64_t m0, int64_t M,
                        float *out, int ldo, void *stream);
/* the query form for B volumes in one launch (round 6; the surface decoders of predict.py:184-187 for a whole batch): volume b = vol + b * vol_bstride
 * floats, its M queries query [b][M][3], its rows out [b][M][ldo].  Alignment as gn_trilinear_sample's per-query form; vol_bstride must keep it for every volume. */
int gn_trilinear_sample_batch(const float *vol, int B, int64_t vol_bstride, int D, int H, int W, int C, const float *query, int64_t M, float *out, int ldo,
                              void *stream);

/* Fused implicit decoder: trilinear sampling (as gn_trilinear_sample) + the 3-layer MLP of ImplicitWNFDecoder
 * (Linear -> ReLU -> BatchNorm1d per layer, widths [C0, N1, N2, OUT]) in one kernel -- networks/conv_implicit_wnf.py:128-149,
 * predict.py:145-157,184-187.  Activations stay in LDS; w1p / w2p are k-pair-major packs Wp[k/2][n][2] of the Linear
 * weights W[n][k]; w3 is [OUT][N2] row-major; (s*, t*) are the folded eval-BatchNorm scale/shift (NULL = no BN).
 * If xin != NULL the rows xin[M][C0] (ld ldxin) are used instead of sampling (two-kernel form: gn_trilinear_sample first).
 * Constraints: C0 % 32 == 0, N1 and N2 multiples of 256, OUT <= 4 (otherwise use gn_trilinear_sample + gn_linear); xin, w1p and w2p 16-byte aligned and
 * ldxin % 4 == 0 (16-byte loads; GN_EINVAL otherwise, before any launch); vol packed fp32, read one float at a time (no alignment beyond a float's).
 * run_if: NULL, or a device float: the launch does nothing unless *run_if != 0 (pairs with gn_implicit_decode_split, which skips
 * the garments gn_decoder_input_scale marks unsafe for the fp16 planes: the choice is made on the device, without a host sync). */
int gn_implicit_decode(const float *vol, int D, int H, int W, int C0, const float *xin, int ldxin, const float *query, int Q, int64_t m0, int64_t M,
                       const float *w1p, const float *b1, const float *s1, const float *t1, int N1, const float *w2p,
                       const float *b2, const float *s2, const float *t2, int N2, const float *w3, const float *b3,
                       const float *s3, const float *t3, int OUT, float *out, int ldo, const float *run_if, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Isosurface.
 * ------------------------------------------------------------------------------------------------------- */

/* Gaussian gradient magnitude (sigma, mode='nearest').  replaces scipy.ndimage.gaussian_gradient_magnitude --
 * predict.py:162-163.  Bit-compatible accumulation order (fp64 taps, fp32 stores).  A kernel radius int(4 sigma + 0.5) <= 2 (the
 * reference's sigma = 0.5) runs as ONE fused launch (tile + halo in LDS, each voxel read once and written once) and does not touch
 * tmp (may be NULL); larger radii run 8 separable passes through tmp: 2 volumes of workspace. */
int gn_ggm3d(const float *vol, int n0, int n1, int n2, double sigma, float *tmp, float *out, void *stream);

/* min / max of a float array (device result [2]); level-range check of skimage marching_cubes (measure/_marching_cubes_lewiner.py: volume.min() /
 * volume.max(): numpy's NaN-propagating reductions -- a NaN anywhere gives NaN in the record, round 6; before: fminf / fmaxf). */
int gn_minmax(const float *x, int64_t n, float *out2, void *stream);
/* the same for `batch` volumes of one shape in one set of launches (one volume per blockIdx.y): vol / out [batch][n0][n1][n2],
 * tmp [2][batch][n0][n1][n2]; x [batch][n] (n % 4 == 0), out2 [batch][2].  What predict.py:160-181 does garment by garment. */
int gn_ggm3d_batch(const float *vol, int batch, int n0, int n1, int n2, double sigma, float *tmp, float *out, void *stream);
int gn_minmax_batch(const float *x, int batch, int64_t n, float *out2, void *stream);
/* gn_ggm3d_batch with two options (round 6; predict.py:160-171 needs the volume's range next to its gradient magnitude):
 *   range2 != NULL  [batch][2]: (min, max) of every volume, NaN-propagating, computed from the values the fused launch stages anyway (its tiles and
 *                   edge-replicated halos are voxels of the volume): every wave leaves one pair in range_ws (gn_ggm3d_range_workspace_bytes() bytes, contents
 *                   scratch), a one-workgroup-per-volume launch folds them -- no pass of its own over the volume, no atomics, equal to gn_minmax_batch bit
 *                   for bit; a kernel radius above 2 (8-pass form) calls gn_minmax_batch and ignores range_ws.
 *   accum_bits      64: scipy's arithmetic (fp64 taps), bit for bit, = gn_ggm3d_batch.  32: the same operation order accumulated in fp32 (fused form
 *                   only): 1e-6-class against scipy, not bit-compatible -- an opt-in for callers that hold floats to a tolerance. */
size_t gn_ggm3d_range_workspace_bytes(int batch, int n0, int n1, int n2);
int gn_ggm3d_batch_ex(const float *vol, int batch, int n0, int n1, int n2, double sigma, float *tmp, float *out, int accum_bits, float *range2,
                      void *range_ws, size_t range_ws_bytes, void *stream);

/* Lewiner marching cubes (MC33).  replaces skimage.measure.marching_cubes(method='lewiner') -- predict.py:172-177.
 * gn_mc33_workspace_bytes: bytes of `ws` for a volume of n0*n1*n2.
 * gn_mc33: classify + scan + emit.  verts [cap_v][3] float32 (array-axis order, voxel units), faces [cap_f][3]
 * int32 ('ascent' orientation), normals [cap_v][3], values [cap_v]; counts_dev[2] = {V, F} (device int64) are
 * always written; entries beyond the capacities are dropped (caller re-runs with larger buffers). */
size_t gn_mc33_workspace_bytes(int n0, int n1, int n2);
int gn_mc33(const float *vol, int n0, int n1, int n2, double level, void *ws, size_t ws_bytes, float *verts,
            int32_t *faces, float *normals, float *values, int64_t cap_v, int64_t cap_f, int64_t *counts_dev,
            void *stream);
/* `batch` volumes of one shape at one level in one set of launches: vol [batch][n0][n1][n2], verts / normals [batch][cap_v][3], faces
 * [batch][cap_f][3], values [batch][cap_v], counts_dev [batch][2]; every volume's result is what gn_mc33 gives for it alone. */
size_t gn_mc33_batch_workspace_bytes(int batch, int n0, int n1, int n2);
int gn_mc33_batch(const float *vol, int batch, int n0, int n1, int n2, double level, void *ws, size_t ws_bytes, float *verts,
                  int32_t *faces, float *normals, float *values, int64_t cap_v, int64_t cap_f, int64_t *counts_dev, void *stream);
/* gn_mc33_batch with its four stages (classify, scan + counts, vertices + normals / values, faces) bracketed by HIP events: the call
 * SYNCHRONISES and fills stage_ms (host float[4], milliseconds).  Measurement hook of bench.py's hbm_members; same results. */
int gn_mc33_batch_profiled(const float *vol, int batch, int n0, int n1, int n2, double level, void *ws, size_t ws_bytes, float *verts,
                           int32_t *faces, float *normals, float *values, int64_t cap_v, int64_t cap_f, int64_t *counts_dev, void *stream,
                           float *stage_ms);

/* out[i] = vol[(uint32)(verts[i]/spacing)] (float64 division, truncation) -- predict.py:179-181.
 * verts_vox: float32 voxel-unit vertices as produced by gn_mc33; spacing applied in fp64 as numpy does. */
int gn_gather_nn(const float *vol, int n0, int n1, int n2, const float *verts_vox, int64_t nv, double spacing,
                 float *out, void *stream);
/* batched: vol [batch][n0][n1][n2], verts_vox [batch][nv][3] (nv rows per volume, padded), out [batch][nv] */
int gn_gather_nn_batch(const float *vol, int batch, int n0, int n1, int n2, const float *verts_vox, int64_t nv, double spacing,
                       float *out, void *stream);

/* verts_out[i] = (float)((double)verts_vox[i] * spacing): the float32 query points predict.py:184 feeds to the
 * surface decoder (mc_verts.astype(np.float32)). */
int gn_scale_verts(const float *verts_vox, int64_t nv, double spacing, float *verts_out, void *stream);

/* Mesh compaction = delete_invalid_verts (common/marching_cubes_util.py:38-52; the hole-prediction head of predict.py:202-209 and
 * eval.py:39): keep the faces whose three vertices are flagged on_surface, keep the vertices those faces use in ascending raw index
 * (np.unique order), renumber the faces.  verts: [V][3] of vert_bytes / 3 byte scalars (12 = float32, 24 = float64); faces [F][3]
 * int32; on_surface [V] bytes (0 / non-0).  out_verts / out_faces must hold V / F rows; counts (device int64[3]) = kept (V', F') and a flag:
 * 1 if some face index was outside [0, V) (numpy raises IndexError there; such a face is dropped without touching memory). */
size_t gn_mesh_compact_workspace_bytes(int64_t V, int64_t F);
int gn_mesh_compact(const void *verts, int vert_bytes, const int32_t *faces, const unsigned char *on_surface, int64_t V, int64_t F,
                    void *ws, size_t ws_bytes, void *out_verts, int32_t *out_faces, int64_t *counts, void *stream);

/* Largest connected component of a triangle mesh = the filter of the reference's hole removal (eval.py:497-503, :536-545:
 * igl.adjacency_matrix + igl.connected_components + np.argmax(cc_sizes), followed by delete_invalid_verts = gn_mesh_compact).  Lock-free
 * union-find over the mesh edges that always hooks the larger root under the smaller: a component's label is its LOWEST vertex index whatever
 * the interleaving (libigl numbers components in that order), and of several largest components the one with the lowest label wins (np.argmax
 * takes the first maximum).  faces [F][3] int32; mask [V] bytes (1 = vertex in the winning component); label [V] int32 or NULL; info = device
 * int64[4]: number of components, size of the winner, its label (-1 for V = 0), 1 if a face index was outside [0, V). */
size_t gn_mesh_largest_component_workspace_bytes(int64_t V);
int gn_mesh_largest_component(const int32_t *faces, int64_t F, int64_t V, void *ws, size_t ws_bytes, unsigned char *mask, int32_t *label,
                              int64_t *info, void *stream);

/* The decoder MLP of gn_implicit_decode for the shipped shape [128, 256, 256, OUT<=4] on the 16-bit matrix cores: fp32 operands
 * split into two fp16 planes (3 MFMA products per fp32 product, fp32 accumulation -- the f16x2 arithmetic of
 * gn_conv3d_gcr_split), activations chained through registers, weights streamed through an LDS ring
 * (csrc/decode_split.hip).  xin: pre-sampled rows [M][ldxin] (gn_trilinear_sample); wpack / tab: weight stages and epilogue
 * tables from garmentnets_amd.ops.pack_decode_split (per-hidden-unit power-of-two weight scales folded in); xscale: NULL or a
 * device record {s, 1/s, unsafe, 0} from gn_decoder_input_scale -- rows and biases are multiplied by s, the output sum by 1/s (exact:
 * ReLU is positively homogeneous), so un-normalised inputs of any magnitude are split at O(1); unsafe != 0: the launch does nothing
 * (run gn_implicit_decode with run_if = &xscale[2] right after it).  A hidden value beyond fp16's range in the
 * scaled units reaches the output as NaN (never as a wrong finite number); callers re-run such a batch with gn_implicit_decode.
 * replaces the three Linear/ReLU/BatchNorm1d blocks of ImplicitWNFDecoder.forward -- networks/conv_implicit_wnf.py:128-149. */
int gn_implicit_decode_split(const float *xin, int ldxin, int64_t M, const void *wpack, const float *tab, const float *xscale,
                             int C0, int N1, int N2, int OUT, float *out, int ldo, void *stream);
/* B row sets of M rows each in ONE launch (round 6): xin [B][M][ldxin], out [B][M][ldo], xscale NULL or [B][4] (one gn_decoder_input_scale record per row set;
 * a set marked unsafe is skipped and left to gn_implicit_decode_batch(run_if = xscale + 2, run_if_stride = 4)).  Row for row the single call's results. */
int gn_implicit_decode_split_batch(const float *xin, int ldxin, int64_t M, int B, const void *wpack, const float *tab, const float *xscale,
                                   int C0, int N1, int N2, int OUT, float *out, int ldo, void *stream);
/* gn_implicit_decode on B sets of M pre-sampled rows (the gated fp32 twin of the call above): run_if NULL or one flag per row set at run_if[b * run_if_stride]. */
int gn_implicit_decode_batch(const float *xin, int ldxin, int64_t M, int B, int C0, const float *w1p, const float *b1, const float *s1, const float *t1,
                             int N1, const float *w2p, const float *b2, const float *s2, const float *t2, int N2, const float *w3, const float *b3,
                             const float *s3, const float *t3, int OUT, float *out, int ldo, const float *run_if, int run_if_stride, void *stream);

/* gn_implicit_decode_split with the lattice sampler INSIDE the decoder kernel (reference call site
 * networks/conv_implicit_wnf.py:137-149 under the lattice loop of predict.py:145-157): rows m0 .. m0+M-1 of the (Q,Q,Q) lattice are sampled
 * (trilinear, border, align_corners: gn_trilinear_sample's arithmetic) from the channel-last volume vol [D][H][W][32] by the kernel that
 * multiplies them -- a tile is a brick of 4 x 8 x 8 lattice points whose voxel box is DMA'd into LDS while the previous brick is multiplied; no
 * sampled-row buffer exists.  Folded scalar decoder only ([32, 256, 256, 1]); D*H*W*128 < 2^32; Q >= D, H, W (the lattice at least as fine as the
 * volume: what bounds a brick's box -- an error otherwise).  Bit-identical to gn_trilinear_sample + gn_implicit_decode_split. */
int gn_implicit_decode_lattice_split(const float *vol, int D, int H, int W, int C0, int Q, int64_t m0, int64_t M, const void *wpack,
                                     const float *tab, const float *xscale, int N1, int N2, int OUT, float *out, int ldo, void *stream);

/* Input scale of gn_implicit_decode_split for B garments from the per-(sample, channel) sums of squares [B][C] (fp64) of the volume
 * the rows are sampled from (V voxels per channel; the statistics gn_conv3d_gcr* emit): s = 2^k with (largest channel rms) * s in
 * [1, 2), clamped to smax (pack_decode_split: keeps the scaled biases below 2^13).  out4: [B][4] = {s, 1/s, unsafe, 0}; unsafe = 1
 * when the clamp costs more than 2^4 (biases dwarf weights x activations: the fp16 planes would lose fp32-class accuracy). */
int gn_decoder_input_scale(const double *sumsq, int64_t V, int B, int C, float smax, float *out4, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Widening: evaluation helpers.
 * ------------------------------------------------------------------------------------------------------- */

/* Exact 1-nearest-neighbour of every query in `ref` (brute force, fp32 squared distance, ties -> lowest index).
 * replaces the scipy cKDTree.query(k=1) calls of the Chamfer metrics -- eval.py:259-263,381-385.
 * idx [nq] int32, d2 [nq] squared distance. */
int gn_nearest_neighbor(const float *query, int64_t nq, const float *ref, int64_t nr, int32_t *idx, float *d2, void *stream);

/* fp64 exact 1-nearest-neighbour for P (query set, reference set) pairs in one launch -- the cKDTree.query(k=1) calls of
 * eval.py:79-80,259-263,381-385 (gradient threshold, chamfer, hybrid chamfer).  query / ref: [*][3] fp64 rows; pairs [P][4] int64 on the
 * device = {q_off, nq, r_off, nr} (rows of query / ref); max_nq = the largest nq.  idx [*] int32 (relative to r_off) and d2 [*] fp64 are
 * written at rows q_off .. q_off + nq - 1.  d2 = (dx*dx + dy*dy) + dz*dz (cKDTree's order); ties -> lowest index; empty reference set ->
 * d2 = +inf, idx = -1.  P <= 65535. */
int gn_nearest_neighbor_f64_batch(const double *query, const double *ref, const int64_t *pairs, int P, int64_t max_nq, int32_t *idx, double *d2,
                                  void *stream);

/* fp64 unsigned squared distance from every query to the nearest triangle of its mesh, P (query set, mesh) pairs in one launch -- libigl's
 * point_mesh_squared_distance, which igl.hausdorff calls in both directions (eval.py:564-567).  verts [*][3] fp64, faces [*][3] int32
 * RELATIVE to the pair's v_off; pairs [P][6] int64 = {q_off, nq, v_off, nv, f_off, nf}.  face_idx [*] int32 (relative to f_off) and d2 [*]
 * fp64 at the query rows.  Ties -> lowest face index; empty mesh -> +inf, -1; a NaN query -> d2 = NaN.  Degenerate triangles (zero area,
 * repeated vertices) are measured as their edges.  A face index outside [0, nv) sets *bad = 1 (caller zeroes it; the distances are then
 * meaningless).  P <= 65535. */
int gn_point_mesh_sqdist_batch(const double *query, const double *verts, const int32_t *faces, const int64_t *pairs, int P, int64_t max_nq,
                               int32_t *face_idx, double *d2, int64_t *bad, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Dataset preparation: the generalised winding number of a triangle mesh (the WNF training target), fp64, all pairs, exact (no hierarchy).
 * Per (query q, face (v0, v1, v2)): a = v0 - q, b = v1 - q, c = v2 - q (one subtraction per component),
 *     la = sqrt((a.x*a.x + a.y*a.y) + a.z*a.z)  (lb, lc alike),  cr = b x c,  num = (a.x*cr.x + a.y*cr.y) + a.z*cr.z,
 *     dab = (a.x*b.x + a.y*b.y) + a.z*b.z  (dbc, dca alike),  den = (((la*lb)*lc + dab*lc) + dbc*la) + dca*lb,
 *     omega = 2 * atan2(num, den)   (Van Oosterom-Strackee),   w(q) = (0 + omega_0 + omega_1 + ...) / (4 pi) in face-index order,
 * every operation rounded on its own (no fma).  A query on a vertex gets atan2(+-0, +0) = +-0 from the incident faces; an empty mesh gives 0.
 * Each value is accumulated by one thread in face order: a pure function of (q, mesh), independent of the launch.
 * ------------------------------------------------------------------------------------------------------- */

/* P (query set, mesh) pairs in one launch, the pairs table of gn_point_mesh_sqdist_batch: query / verts [*][3] fp64, faces [*][3] int32
 * RELATIVE to the pair's v_off, pairs [P][6] int64 on the device = {q_off, nq, v_off, nv, f_off, nf}; max_nq = the largest nq.  out [*] fp64
 * at the query rows.  A face with an index outside [0, nv) sets *bad = 1 (caller zeroes it) and contributes nothing.  P <= 65535. */
int gn_winding_number_batch(const double *query, const double *verts, const int32_t *faces, const int64_t *pairs, int P, int64_t max_nq,
                            double *out, int64_t *bad, void *stream);

/* The winding number of B meshes at every node of a (D, H, W) lattice over the unit cube: node (i, j, k) is the point
 * (i / (D-1), j / (H-1), k / (W-1)), divided in fp64 inside the kernel.  mesh_csr [B + 1][2] int64 on the device = {v_off, f_off}: mesh b
 * owns the vertex rows v_off[b] .. v_off[b+1] - 1 and the face rows f_off[b] .. f_off[b+1] - 1, its face indices relative to v_off[b].
 * out [B][D][H][W] float32 = float(w), rounded once: the bits of float(gn_winding_number_batch at the lattice points).  *bad as above.
 * B <= 65535; D, H, W >= 2; D*H*W < 2^31. */
int gn_winding_field_batch(const double *verts, const int32_t *faces, const int64_t *mesh_csr, int B, int D, int H, int W, float *out,
                           int64_t *bad, void *stream);

/* Dataset preparation: the squared distance from every node of that lattice to each of B meshes (the distance, signed-distance and occupancy
 * training targets are made of it and of the winding field: garmentnets_amd/distance.py).  The lattice, verts, faces and mesh_csr of
 * gn_winding_field_batch.  face_idx [B][D][H][W] int32 (relative to the mesh's first face) and d2 [B][D][H][W] fp64 are the bits
 * gn_point_mesh_sqdist_batch gives at the lattice points: the same operations in the same order, the faces scanned in index order with a
 * strict `<` (ties -> lowest face index), an empty mesh -> (+inf, -1).  Exact and brute force: no hierarchy, no culling.  A face index
 * outside [0, nv) sets *bad = 1 (caller zeroes it) and is never dereferenced.  B <= 65535; D, H, W >= 2; D*H*W < 2^31. */
int gn_distance_field_batch(const double *verts, const int32_t *faces, const int64_t *mesh_csr, int B, int D, int H, int W,
                            int32_t *face_idx, double *d2, int64_t *bad, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Exact volume targets at query points (csrc/query_targets.hip; DESIGN.md "Exact volume targets"; garmentnets_amd/targets.py restates it in numpy):
 * the second stage's gt_volume_value from the garment's mesh alone, for "few queries, many faces" (a training batch: 24 x 6000 queries, ~10 000 faces).
 * A query's fp32 coordinates and the fp32 vertices are widened exactly to fp64; the per-pair arithmetic is gn_winding_number_batch's and
 * gn_point_mesh_sqdist_batch's.  The faces are cut into chunks of GN_QT_FACE_CHUNK consecutive faces (the second grid dimension):
 *     w        each chunk's solid angles added in face order from 0, the chunk sums added in ascending chunk order from 0, the total divided by 4 pi:
 *              the bits of gn_winding_number_batch when F <= GN_QT_FACE_CHUNK, within F * 2^-50 of it otherwise;
 *     d2, face the strict `<` minimum in face order per chunk, then over ascending chunks: the bits of gn_point_mesh_sqdist_batch for every F.
 * With w32 = float(w), the float32 target of `kind`:
 *     GN_QT_WINDING          w32
 *     GN_QT_DISTANCE         float(sqrt(d2)), the root in fp64
 *     GN_QT_SIGNED_DISTANCE  float(clip(1 - 2 * double(w32), -1, 1) * sqrt(d2))
 *     GN_QT_OCCUPANCY        w32 > 0.5f ? 1 : 0
 * then, with use_clip != 0, clip(v / tsdf_clip, -1, 1) (one fp32 division) and, with absolute != 0, |v|: the dataset's data_io steps in their order.
 * An empty mesh gives w = 0, d2 = +inf, face = -1; a NaN query gives NaN (occupancy: 0).  Only the kinds that read w compute solid angles, only those that
 * read d2 compute distances.  One partial per (query, chunk) goes to the workspace and a second launch folds them in ascending chunk order: no atomics, one
 * writer per value, identical calls give identical bits, and a query's result does not depend on B, M, the grid or what else the launch carries.
 * ------------------------------------------------------------------------------------------------------- */
#define GN_QT_FACE_CHUNK 512         /* faces per chunk: a compile-time constant that depends on nothing but itself */
#define GN_QT_WINDING 0              /* volume_group nocs_winding_number_field, sim_nocs_winding_number_field */
#define GN_QT_DISTANCE 1             /* nocs_distance_field */
#define GN_QT_SIGNED_DISTANCE 2      /* nocs_signed_distance_field */
#define GN_QT_OCCUPANCY 3            /* nocs_occupancy_grid */

/* GN_QT_FACE_CHUNK of the built library (what garmentnets_amd/targets.py chunks its numpy sum by) */
int gn_query_targets_face_chunk(void);
/* bytes of workspace for B query sets of M queries against meshes of at most max_nf faces: B * max(1, cdiv(max_nf, GN_QT_FACE_CHUNK)) * M * (8 for w + 12
 * for (d2, face), as `kind` reads them); 0 for an unknown kind or an empty launch */
size_t gn_query_targets_workspace_bytes(int B, int64_t M, int64_t max_nf, int kind);
/* query [B][M][3] fp32; verts [*][3] fp32, faces [*][3] int32 and mesh_csr [B + 1][2] int64 on the device as gn_winding_field_batch reads them (mesh b owns
 * the vertex rows v_off[b] .. v_off[b+1] - 1 and the face rows f_off[b] .. f_off[b+1] - 1, its face indices relative to v_off[b]); max_nf >= the largest
 * face count.  target [B][M] fp32; w, d2 [B][M] fp64 and face_idx [B][M] int32 (relative to the mesh's first face): optional (NULL), written when `kind`
 * computes them.  bad [2] int64 (caller zeroes it): bad[0] = 1 when a face index lies outside [0, nv) (never dereferenced), bad[1] = 1 when a mesh has
 * more than max_nf faces (it is then not walked).  Refused by name before any launch: null pointers, an unknown kind, a short workspace, B > 65535,
 * M >= 2^31, max_nf > 65535 * GN_QT_FACE_CHUNK. */
int gn_query_targets_batch(const float *query, const float *verts, const int32_t *faces, const int64_t *mesh_csr, int B, int64_t M, int64_t max_nf, int kind,
                           int use_clip, float tsdf_clip, int absolute, void *ws, size_t ws_bytes, float *target, double *w, double *d2, int32_t *face_idx,
                           int64_t *bad, void *stream);

/* ---------------------------------------------------------------------------------------------------------
 * Validation losses (networks/pointnet2_nocs.py:257-440, networks/conv_implicit_wnf.py:405-452).
 * Per-element terms in fp32 as torch computes them; sums in fp64.  Deterministic: one plain store of a partial per workgroup into ws,
 * then a fold launch in a fixed order (no atomics: two identical calls give identical bits).  The set / segment tables are HOST arrays
 * (the `_host` suffix); the pointers in them are device pointers.
 * ------------------------------------------------------------------------------------------------------- */
#define GN_LOSS_MAX_SETS 8
#define GN_LOSS_L2 0
#define GN_LOSS_SMOOTH_L1 1
#define GN_LOSS_BCE_LOGITS 2
#define GN_LOSS_ROW_NORM 3   /* |pred - target| of (count, 3) rows: the regression head's error distance */

typedef struct {
    const float *logits;   /* [n][ldl] rows, the first bins * 3 laid out (bins, 3) as gn_nocs_head reads them */
    const float *gt;       /* [n][3] target NOCS coordinates */
    int64_t n;             /* rows, >= 1 */
    int ldl;               /* >= bins * 3 */
    int pad;
} GnNocsBinSet;

typedef struct {
    const float *pred;     /* [count] ([count][3] for GN_LOSS_ROW_NORM) */
    const float *target;   /* same size as pred */
    int64_t count;         /* >= 0 elements (rows for GN_LOSS_ROW_NORM); a multiple of 3 when mirror is set on an element-wise kind */
    int kind;              /* GN_LOSS_L2 | GN_LOSS_SMOOTH_L1 (beta 1) | GN_LOSS_BCE_LOGITS (max(x,0) - x*y + log1p(exp(-|x|))) | GN_LOSS_ROW_NORM
                              (fp32 sqrt((dx*dx + dy*dy) + dz*dz)) */
    int mirror;            /* 1: also sum against the x-mirrored target of (count/3, 3) rows (components/loss.py MirrorMSELoss) */
} GnLossSegment;

/* Binned NOCS head metrics for 1..GN_LOSS_MAX_SETS row sets in one launch (the per-point logits and the global grip-point logits).
 * Per (row, axis): max-subtracted log-sum-exp over the bins; cross entropy at the target bin of gt and at the target bin of the mirrored gt
 * (mirror_axis 0..2: (p - 0.5) * -1 + 0.5 on that axis in fp32; -1: no mirror, the two are equal); first-maximum arg-max -> coordinate as
 * gn_nocs_head.  Target bins are VirtualGrid.get_points_grid_idxs' exactly: fp32 p * (bins - 1), truncation, clamp to [0, bins - 1].
 * out [nsets][4] fp64 = {sum CE, sum CE mirrored, sum |pred - gt|, sum |pred - gt mirrored|} (the norms fp32 per row).  bins >= 1. */
size_t gn_nocs_bin_metrics_workspace_bytes(const GnNocsBinSet *sets_host, int nsets);
int gn_nocs_bin_metrics(const GnNocsBinSet *sets_host, int nsets, int bins, int mirror_axis, void *ws, size_t ws_bytes, double *out, void *stream);

/* Element-wise loss sums for 1..GN_LOSS_MAX_SETS segments in one launch (volume / surface / mc-surface decoders, the regression head).
 * out [nsegs][2] fp64 = {sum of the terms, sum against the x-mirrored target (0 unless the segment's mirror is set)}. */
size_t gn_value_losses_workspace_bytes(const GnLossSegment *segs_host, int nsegs);
int gn_value_losses(const GnLossSegment *segs_host, int nsegs, void *ws, size_t ws_bytes, double *out, void *stream);

/* ---- Loss gradients (csrc/losses.hip): the backward of the two launches above, for a training step.  Both read the forward's fp64 sums FROM THE
 * DEVICE and take the mirror decision there (every thread the same fp64 comparison; no host branch between forward and backward).  `upstream` is a
 * device pointer to the fp32 gradient of the scalar loss.  Every output element is written exactly once with a plain store (no atomics). */
typedef struct {
    const float *logits;   /* [n][ldl] rows, the first bins * 3 laid out (bins, 3) */
    const float *gt;       /* [n][3] */
    float *grad;           /* [n][ldg] out: columns [0, bins * 3) the gradient, [bins * 3, ncols) zero */
    int64_t n;             /* rows, >= 1 */
    int ldl;               /* >= ncols */
    int ldg;               /* >= ncols */
    int ncols;             /* >= bins * 3: the columns of a (padded) logits row */
    int pad;
} GnNocsBinGradSet;

typedef struct {
    const float *pred;     /* [count] */
    const float *target;   /* [count] */
    float *grad;           /* [count] out */
    int64_t count;         /* >= 0; a multiple of 3 when mirror is set */
    double coef;           /* weight_s / count_s of a mean-reduced loss */
    int kind;              /* GN_LOSS_L2 | GN_LOSS_SMOOTH_L1 | GN_LOSS_BCE_LOGITS; GN_LOSS_ROW_NORM is a metric and is refused */
    int mirror;
} GnLossGradSegment;

/* grad[r][k * 3 + ax] = (softmax_k(logits[r][. * 3 + ax]) - [k == target bin]) * weights_host[s] / (3 n_s) * upstream, fp32.  The softmax is the
 * forward's max-subtracted one; the target bin is the forward's (mirrored on mirror_axis for the WHOLE batch iff the mirrored weighted loss
 * sum_s w_s * sums[s][1] / (3 n_s) is strictly smaller than the plain one over sums[s][0]).  sums: gn_nocs_bin_metrics' out, on the device. */
int gn_nocs_bin_loss_bwd(const GnNocsBinGradSet *sets_host, int nsets, int bins, int mirror_axis, const double *sums, const double *weights_host,
                         const float *upstream, void *stream);

/* grad[e] = d term(pred[e], target[e]) / d pred[e] * coef_s * upstream, fp32: 2 d (l2); d clamped to [-1, 1] (smooth_l1: torch's choice, the quadratic
 * branch at |d| == 1, 0 at d == 0); sigmoid(p) - t (bce_logits).  A mirrored segment differentiates against the x-mirrored target iff ITS mirrored sum
 * sums[s][1] is strictly smaller than sums[s][0] (MirrorMSELoss, per segment).  sums: gn_value_losses' out, on the device. */
int gn_value_losses_bwd(const GnLossGradSegment *segs_host, int nsegs, const double *sums, const float *upstream, void *stream);

/* ---- Fused Adam (csrc/optim.hip): torch.optim.Adam's update (L2 weight decay g + wd * p) of every tensor of a device table in ONE launch.
 * table: DEVICE array of n entries sorted by blk0; entry e owns the workgroups [blk0_e, blk0_e + ceil(numel_e / GN_ADAM_CHUNK)) and workgroup
 * j of them the elements [j * GN_ADAM_CHUNK, min((j + 1) * GN_ADAM_CHUNK, numel_e)).  hyper_host: 1..GN_ADAM_MAX_HYPER sets of scalars, the bias
 * corrections computed by the caller in fp64 from the step count.  Each element is read and written once, 16 bytes at a time where all four pointers
 * of the tensor are 16-byte aligned; the per-element arithmetic (fp64 of the fp32 operands, each result rounded once) is one function whatever the
 * path.  No atomics.  More workgroups than one grid holds are split over launches. */
#define GN_ADAM_CHUNK 4096
#define GN_ADAM_MAX_HYPER 16
typedef struct {
    float *p;              /* [numel] parameter, updated in place */
    const float *g;        /* [numel] gradient */
    float *exp_avg;        /* [numel] updated in place */
    float *exp_avg_sq;     /* [numel] updated in place */
    int64_t numel;         /* >= 1 */
    int64_t blk0;          /* first workgroup of this entry */
    int hyper;             /* index into hyper_host */
    int pad;
} GnAdamEntry;

typedef struct {
    double lr, beta1, beta2, eps, weight_decay;
    double bias_correction1;        /* 1 - beta1 ^ step */
    double bias_correction2_sqrt;   /* sqrt(1 - beta2 ^ step) */
} GnAdamHyper;

int gn_adam_step(const GnAdamEntry *table, int n, int64_t nblocks, const GnAdamHyper *hyper_host, int nhyper, void *stream);

/* ---- Gradient pack (csrc/optim.hip): every gradient of a device table into ONE flat fp32 buffer, divided by the world size, in ONE launch -- the
 * buffer a data-parallel step hands to one all-reduce (sum), whose result is then the mean over the ranks (garmentnets_amd/parallel.py).
 * table: DEVICE array of n_entries entries sorted by blk0; entry e owns the workgroups [blk0_e, blk0_e + ceil(numel_e / GN_ADAM_CHUNK)) and the floats
 * [dst_off_e, dst_off_e + ceil4(numel_e)) of flat: dst_off_e % 4 == 0, the ranges of two entries do not overlap, and the kernel writes zeros from numel_e up
 * to the next multiple of 4.  src == NULL writes zeros over the whole range.  Value written: src[i] for world == 1 (the bits), __fdiv_rn(src[i], world)
 * otherwise.  src needs a float's alignment only: a slice of it that starts 16-byte aligned is read in 16-byte loads, any other element by element (no
 * alignment beyond a float's is assumed); every store is 16 bytes wide.  No atomics, one writer per element, and no store at or beyond flat_numel whatever the table says.
 * GN_EINVAL before any launch: a null table or flat, n_entries < 1, world < 1, n_blocks outside [1, 2^31), flat_numel not a multiple of 4, flat not
 * 16-byte aligned. */
typedef struct {
    const void *src;       /* [numel] fp32 gradient, or NULL: zeros */
    int64_t dst_off;       /* first float of this entry in flat, a multiple of 4 */
    int64_t numel;
    int64_t blk0;          /* first workgroup of this entry */
} GnPackEntry;

int gn_grad_pack(const GnPackEntry *table, int n_entries, int64_t n_blocks, float *flat, int64_t flat_numel, int world, void *stream);

/* ---- Operator gradients (csrc/grad.hip): fp32 in / fp32 out.  The selections (grid scatter max / min, segment max, global max pool) hand an output
 * element's gradient to ONE input element: the one whose value is bit-equal to the forward's stored output, the lowest point / edge index among equal
 * values; a NaN never wins.  The sums (sa_gather, knn_interpolate, the sampler's volume gradient) are ordered: one owner per destination adds its
 * terms in ascending element index, so identical calls give identical bits; no float atomics anywhere. */

/* Gradient of gn_grid_scatter / _ex: grad_src[p][c] = grad_vol[cell(p)][c] * k, k = 1 (sum), 1 / count(cell) (mean), and for max / min 1 for the
 * winning point of (cell, c), else 0.  vol (the forward's output), src / lds: read for max and min only (NULL otherwise).  Channels [c_real, C) are
 * pads: gradient 0.  reduce 4 (mul) is refused.  A point whose cell is outside [0, cells) gets 0.  ws: gn_grid_scatter_bwd_workspace_bytes. */
size_t gn_grid_scatter_bwd_workspace_bytes(int64_t N, int C, int64_t cells, int reduce);
int gn_grid_scatter_bwd(const float *grad_vol, const float *vol, const float *src, int lds, const int32_t *flat_idx, int64_t N, int C, int c_real,
                        int64_t cells, int reduce, void *ws, size_t ws_bytes, float *grad_src, int ldg, void *stream);

/* Gradient of gn_segment_max: grad_in[c*S+s][ch] = grad_out[c][ch] for the first valid slot s that holds out[c][ch], else 0 (every row is written). */
int gn_segment_max_bwd(const float *grad_out, int ldg, const float *out, int ldo, const float *in, int ldi, const int32_t *slot_src, int M, int S,
                       int C, float *grad_in, int ldgi, void *stream);

/* Gradient of gn_global_max_pool: the same per example (rows ptr[b]..ptr[b+1], the lowest row among equal values). */
int gn_global_max_pool_bwd(const float *grad_out, int ldg, const float *out, int ldo, const float *in, int ldi, const int32_t *ptr, int B, int C,
                           float *grad_in, int ldgi, void *stream);

/* Gradient of gn_sa_gather with respect to x: grad_x[j][:C] = sum of grad_edge[e][:C] over the edge rows e whose source is j, in ascending e.
 * slot_src [rows]: gn_sa_gather's record of every row's source (after the self-loop rule; -1 = empty slot).  Every row of grad_x is written. */
size_t gn_sa_gather_bwd_workspace_bytes(int64_t rows, int64_t n_points);
int gn_sa_gather_bwd(const float *grad_edge, int lde, const int32_t *slot_src, int64_t rows, int C, int64_t n_points, void *ws, size_t ws_bytes,
                     float *grad_x, int ldgx, void *stream);

/* The neighbours gn_knn_interpolate / _any use (ascending (d2, index), any k >= 1): nbr [Nq][k] int32 (-1 past an example's sources), d2 [Nq][k]. */
int gn_knn_neighbours(const float *ps, const int32_t *ptr_s, const float *pq, const int32_t *ptr_q, int B, int Nq, int k, int32_t *nbr, float *d2,
                      void *stream);
/* Gradient of gn_knn_interpolate / _any with respect to the source features: grad_xs[j] = sum over the (query i, rank r) pairs with nbr[i][r] == j,
 * in ascending (i, r), of (w_ir / sum_r' w_ir') grad_y[i], w = 1 / max(d2, 1e-16).  The search and the weights are data (no gradient to positions). */
size_t gn_knn_interpolate_bwd_workspace_bytes(int64_t Nq, int k, int64_t Ns);
int gn_knn_interpolate_bwd(const int32_t *nbr, const float *d2, int Nq, int k, const float *grad_y, int ldg, int Ns, int C, void *ws, size_t ws_bytes,
                           float *grad_xs, int ldgx, void *stream);

/* Gradient of gn_trilinear_sample / _batch (border padding, align_corners=True).  grad_rows: (B M) rows of ldg floats; vol: B dense channel-last
 * volumes; query (B, M, 3).  grad_vol (B, D, H, W, C) dense, every voxel written: the corner weights times grad_rows, summed per voxel in ascending
 * (query, corner).  grad_query (B, M, 3): F.grid_sample's rule -- a coordinate clamped at the border gets 0.  Either may be NULL (not computed). */
size_t gn_trilinear_sample_bwd_workspace_bytes(int B, int64_t M, int D, int H, int W);
int gn_trilinear_sample_bwd(const float *grad_rows, int ldg, const float *vol, int B, int D, int H, int W, int C, const float *query, int64_t M,
                            void *ws, size_t ws_bytes, float *grad_vol, float *grad_query, void *stream);

/* ---- UNet gradients (csrc/unet_grad.hip; DESIGN.md "UNet gradients").  Channel-last [B][D][H][W][C] fp32, the stored (channel-padded) layout of the
 * forward.  No float atomics: every sum has a fixed order, identical calls give identical bits. ---- */

/* Weight gradient of one GroupNorm -> Conv3d(3x3x3, pad 1) -> ReLU layer: dw[co][ci][kd][kh][kw] (nn.Conv3d's layout over the STORED widths,
 * Cin = C0 + C1) = sum over (b, voxel) of xn[b][voxel + tap][ci] * g[b][voxel][co], xn = x*a + d inside the volume and 0 in the padding over the virtual
 * concat [src0 (C0, full res), src1 (C1, half res, nearest-upsampled)] -- gn_conv3d_gcr's operand -- and g = dy where y > 0, else 0 (y NULL: g = dy).
 * a, d: [B][Cin].  C0, C1 multiples of 4, Cout of 32.  Workspace: chains x 27 x round_up(Cin, 32) x Cout floats, where the B * ceil(D/4) * ceil(H/8) *
 * ceil(W/8) tiles are cut into chains = ceil(tiles / ceil(tiles / min(tiles, ceil(512 / blocks)))) runs, blocks = ceil(Cin/32) * Cout / (Cout % 64 ? 32 : 64). */
size_t gn_conv3d_bwd_weight_workspace_bytes(int B, int D, int H, int W, int Cin, int Cout);
int gn_conv3d_bwd_weight(const float *src0, int C0, const float *src1, int C1, const float *a, const float *d, const float *y, const float *dy,
                         int B, int D, int H, int W, int Cout, void *ws, size_t ws_bytes, float *dw, void *stream);

/* g = y > 0 ? dy : 0 over n floats (n % 4 == 0); g may be dy.  The data gradient of the layer is gn_conv3d_gcr(g) with the flipped / transposed pack. */
int gn_relu_mask(const float *y, const float *dy, int64_t n, float *g, void *stream);

/* ---- f16x2 backward of the UNet convolutions (csrc/unet_grad_split.hip; DESIGN.md "f16x2 backward of the UNet convolutions").  Opt-in
 * (arith.Arith.conv_grad_mode = "f16x2"); the same mathematical objects as the fp32 entries above on the 16-bit matrix cores: operands split into two
 * fp16 planes after a power-of-two scale, the products hi*hi, hi*lo, lo*hi on v_mfma_f32_32x32x16_f16, fp32 accumulation.  No float atomics. ---- */

/* gn_relu_mask over B samples of n floats each (n % 4 == 0; y NULL: g = dy), and on the way gmax[b] = the largest FINITE |g| of sample b (0 for an
 * all-zero sample; an Inf / NaN never decides a scale).  scale / inv (both or neither): scale[b][0..C) = 2^k[b], inv[b] = 2^-k[b] with
 * gmax[b] * 2^k[b] in [2^14, 2^15) (k = 0 for an all-zero sample, held to [-126, 126]) -- the a (with d = 0) and act_inv_scale that gn_conv3d_gcr_split
 * takes for the DATA gradient: the direct GN_SPLIT_F16X2 form on the pack of the flipped / transposed weight, no ReLU.  Two launches (a partial
 * maximum per workgroup in the workspace, then one workgroup per sample), no atomics; nothing is read back. */
size_t gn_relu_mask_max_workspace_bytes(int B);
int gn_relu_mask_max(const float *y, const float *dy, int B, int64_t n, int C, float *g, float *gmax, float *scale, float *inv, void *ws,
                     size_t ws_bytes, void *stream);

/* gn_conv3d_bwd_weight on fp16 planes.  Same operands, layout, chains and fixed summation order (the chain count is gn_conv3d_bwd_weight's; the
 * workspace holds a header of ceil((16 + 4 B) / 256) * 256 bytes in front of the partials and must be 16-byte aligned).  Scales, one power of two per
 * operand per LAUNCH (a chain may span samples), found on the device and undone exactly when the chains are folded:
 *   a, d, x_inv: the forward's operand as gn_conv3d_gcr_split takes it -- a and d multiplied by the sample's power of two, x_inv[b] its inverse
 *                (gn_groupnorm_affine's act_inv_scale); the launch scale is 1 / max_b x_inv[b].  x_inv NULL: a, d as gn_conv3d_bwd_weight takes them, the
 *                operand's range is the caller's (|x a + d| < 65504)
 *   gmax [B]:    the largest finite |g| per sample (gn_relu_mask_max); g is scaled so that the batch maximum lies in [2^14, 2^15)
 * All-zero dy: exact zeros.  An Inf / NaN in g: every dw entry of that output channel is non-finite. */
size_t gn_conv3d_bwd_weight_split_workspace_bytes(int B, int D, int H, int W, int Cin, int Cout);
int gn_conv3d_bwd_weight_split(const float *src0, int C0, const float *src1, int C1, const float *a, const float *d, const float *x_inv, const float *y,
                               const float *dy, const float *gmax, int B, int D, int H, int W, int Cout, void *ws, size_t ws_bytes, float *dw,
                               void *stream);

/* nn.GroupNorm's backward over the virtual concat, per source.  dxn: the gradient at the conv's operand, [B][fine voxels][ldg], this source's channels at
 * column goff.  x: the source as stored, [B][D][H][W][C] at its own resolution; half != 0: x is the half-resolution source (fine = 2D x 2H x 2W) and the 8
 * fine gradients of a coarse voxel are added first in ascending (dz, dy, dx) order.
 * _stats: s1[b][c] = sum dxn, s2[b][c] = sum dxn * x, fp64.  Workspace: B * ceil(D*H*W / 512) * 2 * C doubles.
 * _coef:  from those sums (t1_k, t2_k: [B][Sk]), the forward's statistics (sumk, sqk: [B][Sk], Vk voxels) and gamma [C0 + C1] (Ck real channels in rows of
 *         Sk stored ones, groups over the real channels, as gn_groupnorm_affine_map): p, q, r [B][S0 + S1] with dx = dxn*p + x*q + r (0 on the pads),
 *         dgamma, dbeta [C0 + C1] summed over the samples in ascending order.
 * _apply: dx = dxn*p + x*q + r; half: dx[coarse] = sum8(dxn)*p + 8*x*q + 8*r.  p / q / r rows of cs floats, this source at column coff.  accumulate != 0:
 *         added to what dx holds. */
size_t gn_groupnorm_bwd_stats_workspace_bytes(int B, int64_t V, int C);
int gn_groupnorm_bwd_stats(const float *dxn, int ldg, int goff, const float *x, int B, int D, int H, int W, int C, int half, void *ws, size_t ws_bytes,
                           double *s1, double *s2, void *stream);
int gn_groupnorm_bwd_coef(const double *t1_0, const double *t2_0, const double *sum0, const double *sq0, int C0, int S0, int64_t V0, const double *t1_1,
                          const double *t2_1, const double *sum1, const double *sq1, int C1, int S1, int64_t V1, int rep1, int B, int groups, float eps,
                          const float *gamma, float *p, float *q, float *r, float *dgamma, float *dbeta, void *stream);
int gn_groupnorm_bwd_apply(const float *dxn, int ldg, int goff, const float *x, int B, int D, int H, int W, int C, int half, const float *p, const float *q,
                           const float *r, int cs, int coff, int accumulate, float *dx, void *stream);

/* Gradient of gn_maxpool3d_2 (even D, H, W).  The winner of each 2x2x2 window is found again from the stored input by ATen's scan: (z, y, x) order, the
 * first of equal maxima, a NaN beats every number (and a later NaN an earlier one).  grad_in: every voxel written, the losers 0. */
int gn_maxpool3d_2_bwd(const float *grad_out, const float *in, int B, int D, int H, int W, int C, float *grad_in, void *stream);

/* ---- MLP gradients (csrc/linear_grad.hip; DESIGN.md "MLP gradients").  One block of components/mlp.py is r = relu(x W^T + b), y = fadd(fmul(r, sc), sh)
 * with (sc, sh) the folded eval-mode BatchNorm; the UNet's final 1x1x1 convolution is such a block without ReLU and BatchNorm.  Row-major fp32 rows
 * with their own strides.  No float atomics: every sum has a fixed order that depends on the shapes alone, identical calls give identical bits. ---- */

#define GN_LINEAR_BWD_CHUNK_ROWS 512   /* R: gn_linear_bwd_weight's row chunk = the length of its fp32 fma chains */
#define GN_LINEAR_ACT_CHUNK_ROWS 1024  /* gn_linear_act_bwd's row chunk */

/* The epilogue's backward over dy [M][N] and the saved r [M][N]: g[m][n] = r > 0 ? fmul(dy, sc[n]) : 0 (a NaN in r takes no gradient; sc NULL: scale 1;
 * r NULL: no mask; g may be dy, and may be NULL when r and sc both are -- g is dy then), and sums[3][N] fp64 = sum_m g (the bias gradient), sum_m dy (the
 * shift gradient), sum_m dy * r (the scale gradient; products exact; zeros when r is NULL).  Rows in chunks of GN_LINEAR_ACT_CHUNK_ROWS: inside a chunk
 * four interleaved row groups, each ascending, added in ascending order; the chunks in eight contiguous runs, each ascending, the run sums added in
 * ascending order.  M == 0: zeros.  Workspace: ceil(M / GN_LINEAR_ACT_CHUNK_ROWS) * 3 * N doubles. */
size_t gn_linear_act_bwd_workspace_bytes(int64_t M, int N);
int gn_linear_act_bwd(const float *dy, int lddy, const float *r, int ldr, const float *sc, int64_t M, int N, float *g, int ldg, void *ws, size_t ws_bytes,
                      double *sums, void *stream);

/* dW[n][k] = sum_m g[m][n] * x[m][k] on the fp32 matrix cores (v_mfma_f32_32x32x2_f32): per chunk of GN_LINEAR_BWD_CHUNK_ROWS rows one fp32 fma chain
 * over the rows in ascending order, the chunk partials (ws[chunk][N][K], plain stores) added in fp64 -- eight contiguous runs of chunks, each ascending,
 * the run sums in ascending order -- and rounded once.  Any M >= 0, N, K >= 1, ldg >= N, ldx >= K, lddw >= K; float4 loads when ldg, ldx are multiples
 * of 4 and g, x 16-byte aligned.  Rows beyond M and columns beyond N / K are never read.  M == 0: exact zeros.
 * Workspace: ceil(M / GN_LINEAR_BWD_CHUNK_ROWS) * N * K floats. */
size_t gn_linear_bwd_weight_workspace_bytes(int64_t M, int N, int K);
int gn_linear_bwd_weight(const float *g, int ldg, const float *x, int ldx, int64_t M, int N, int K, void *ws, size_t ws_bytes, float *dW, int lddw,
                         void *stream);

/* y[m][n] = fadd(fmul(r[m][n], sc[n]), sh[n]): gn_linear's BatchNorm epilogue as a pass of its own, the same two roundings (y may be r). */
int gn_row_affine(const float *r, int ldr, const float *sc, const float *sh, int64_t M, int N, float *y, int ldy, void *stream);

/* ---- Train-mode BatchNorm of an MLP block (DESIGN.md "Train-mode BatchNorm"): y = (r - mean) * inv * gamma + beta with the batch's own statistics over
 * the M rows of r = relu(x W^T + b).  Three fp64 column reductions of one kernel.  Rows in chunks of GN_LINEAR_ACT_CHUNK_ROWS; inside a chunk 256 / cw
 * interleaved row groups (cw = the power of two >= N, at most 64), each ascending, added by a halving tree; the chunks in eight contiguous runs, each
 * ascending, the run sums added in ascending order.  M == 0: zeros.  Rows beyond M and columns beyond N are never read. ---- */

/* moments[2][N] fp64: the column mean and m2 = sum_m (r - mean)^2 (biased variance m2 / M, unbiased m2 / (M - 1)).  Two passes: mean = (sum_m r) / M, then
 * the squares of the fp64 differences from that mean.  Guarantee, u = 2^-53: |mean - exact| = d <= M u mean_m |r| + u |mean|, and
 * |m2 - exact| <= (M + 4) u m2 + M d^2 (the second term: the computed mean is not the exact one; (M u)^2 mean|r|^2 / variance relative to m2).  A column of
 * equal entries c gives mean == c and m2 == 0.0 exactly while M < 2^29 (every partial sum k c is an fp64 number, and (M c) / M is c).
 * Workspace: ceil(M / GN_LINEAR_ACT_CHUNK_ROWS) * N doubles. */
size_t gn_col_moments_workspace_bytes(int64_t M, int N);
int gn_col_moments(const float *r, int ldr, int64_t M, int N, void *ws, size_t ws_bytes, double *moments, void *stream);

/* dots[2][N] fp64 = sum_m dy, sum_m dy * r (products exact).  Nothing else is written.  Workspace: ceil(M / GN_LINEAR_ACT_CHUNK_ROWS) * 2 * N doubles. */
size_t gn_col_dots_workspace_bytes(int64_t M, int N);
int gn_col_dots(const float *dy, int lddy, const float *r, int ldr, int64_t M, int N, void *ws, size_t ws_bytes, double *dots, void *stream);

/* The backward through the batch statistics and the ReLU: g[m][n] = r > 0 ? (float)((a[n] * dy + b[n] * r) + c[n]) : 0, coef[3][N] = (a, b, c) fp64, each
 * operation in fp64 without contraction, rounded once to fp32 (a NaN in r takes no gradient; g may be dy), and sum_g[N] fp64 = sum_m g (the bias
 * gradient).  Workspace: ceil(M / GN_LINEAR_ACT_CHUNK_ROWS) * N doubles. */
size_t gn_bn_train_bwd_workspace_bytes(int64_t M, int N);
int gn_bn_train_bwd(const float *dy, int lddy, const float *r, int ldr, const double *coef, int64_t M, int N, float *g, int ldg, void *ws, size_t ws_bytes,
                    double *sum_g, void *stream);

/* ---- Resident dataset (csrc/resident.hip; DESIGN.md "Resident dataset"): a training batch assembled on the device.  The samples of a subset are packed
 * into the arrays of a GnResidentStore (ragged parts back to back, their starts in `meta`); the host draws every random number and uploads them; one garment
 * per blockIdx.y reads its sample through the DEVICE index table slots[B] (a slot outside [0, n) writes nothing).  A fixed number of launches per batch, no
 * atomics, explicit _rn arithmetic in numpy's order: identical calls give identical bits.  rot: [B][3][3] fp32 rotation matrices, NULL = none. ---- */

#define GN_RESIDENT_META 10          /* int64 columns of GnResidentStore.meta */
#define GN_RESIDENT_PC_OFF 0         /* first row of the sample in pc_* */
#define GN_RESIDENT_PC_LEN 1         /* its stored cloud length */
#define GN_RESIDENT_VERT_OFF 2       /* first row in sim_verts / nocs_verts / task_verts */
#define GN_RESIDENT_FACE_OFF 3       /* first row in faces, first entry in cdf_nocs / cdf_task */
#define GN_RESIDENT_NUM_FACES 4
#define GN_RESIDENT_MC_VERT_OFF 5    /* first row in mc_verts / mc_flags */
#define GN_RESIDENT_MC_FACE_OFF 6    /* first row in mc_faces, first entry in cdf_mc */
#define GN_RESIDENT_NUM_MC_FACES 7
#define GN_RESIDENT_DATASET_IDX 8
#define GN_RESIDENT_SCALE_BITS 9     /* the 8 bytes of the sample's `scale` */

typedef struct {
    const float *pc_sim, *pc_nocs;   /* [sum N][3] */
    const uint8_t *pc_rgb;           /* [sum N][3] */
    const float *sim_verts, *nocs_verts, *task_verts; /* [sum V][3]; task_verts: the AABBGripNormalizer'd simulation vertices (task space), else NULL */
    const int32_t *faces;            /* [sum F][3], vertex numbers within the sample */
    const double *cdf_nocs, *cdf_task; /* [sum F]: the face-area CDF RandomState.choice searches, of the NOCS / the task-space mesh */
    const float *mc_verts, *mc_flags; /* [sum MV][3], [sum MV]: the marching-cubes mesh and is_vertex_on_surface as 0 / 1 */
    const int32_t *mc_faces;         /* [sum MF][3] */
    const double *cdf_mc;            /* [sum MF] */
    const float *volume;             /* [n][D][H][W] */
    const int64_t *meta;             /* [n][GN_RESIDENT_META] */
    const float *grip;               /* [n][6]: the grip vertex in simulation space, in NOCS space */
    const float *aabb;               /* [2][3]: the store's cloth_aabb_union */
    int32_t n, D, H, W;
} GnResidentStore;

/* the selected rows sel[B][P] (indices into the sample's stored cloud) -> x = rgb / 255, y, pos [B*P][3] fp32 and batch[B*P] = garment.  noise [B][P][3]
 * fp64 or NULL: pos = double(pos) + noise, and the rotation (p.x*R[j][0] + p.y*R[j][1]) + p.z*R[j][2] then runs in fp64, rounded once; without noise in fp32. */
int gn_resident_points(const GnResidentStore *store, const int32_t *slots, int B, int P, const int32_t *sel, const double *noise, const float *rot, float *x,
                       float *y, float *pos, int64_t *batch, void *stream);
/* per garment: grip_pc_idx = the first selected row minimising fp32 sqrt((dx*dx + dy*dy) + dz*dz) to the simulation grip point (stored positions: no noise,
 * no rotation), sim_grip [B][3] (rotated), nocs_grip [B][3], scale_bits, dataset_idx [B], aabb [B][2][3], rot_out [B][3][3] (identity when rot is NULL) */
int gn_resident_garment(const GnResidentStore *store, const int32_t *slots, int B, int P, const int32_t *sel, const float *rot, int64_t *grip_pc_idx,
                        float *sim_grip, float *nocs_grip, int64_t *scale_bits, int64_t *dataset_idx, float *aabb, float *rot_out, void *stream);
/* M volume queries per garment: the first n_uniform are uniform[B][n_uniform][3]; the others a point of the NOCS mesh (face = upper bound of face_u in
 * cdf_nocs; uv [..][2] flipped when u + v >= 1; barycentric_interpolation's fp64 -> fp32 accumulation) plus noise [..][3] in fp64, rounded to fp32 and clipped
 * to [0, 1] (face_u, uv, noise: [B][M - n_uniform] rows).  value [B][M] = the garment's volume there, trilinear in fp32 in ATen's CPU order (corner weight
 * (w_W*w_H)*w_D, corners added in (D, H, W) bit order, those past the far face skipped); occupancy != 0: value > 0.1 as 0 / 1.  rot: the queries turn about
 * (0.5, 0.5, 0) AFTER the values are taken (task space). */
int gn_resident_volume(const GnResidentStore *store, const int32_t *slots, int B, int M, int n_uniform, const float *uniform, const double *face_u,
                       const double *uv, const double *noise, const float *rot, int occupancy, float *query, float *value, void *stream);
/* the M queries of gn_resident_volume alone, bit for bit (exact targets: the store holds no volume).  plain [B][M][3] or NULL: the queries before `rot`
 * turns them, what gn_resident_query_targets evaluates; query [B][M][3]: turned about (0.5, 0.5, 0) when rot != NULL, else the plain ones. */
int gn_resident_volume_queries(const GnResidentStore *store, const int32_t *slots, int B, int M, int n_uniform, const float *uniform, const double *face_u,
                               const double *uv, const double *noise, const float *rot, float *plain, float *query, void *stream);
/* gn_query_targets_batch on the resident meshes: garment b is sample slots[b], its faces store->faces and its vertices store->nocs_verts (task_space != 0:
 * store->task_verts) through the store's own meta rows; total_verts: the rows of the store's vertex arrays; query [B][M][3] (un-turned), value [B][M]. */
int gn_resident_query_targets(const GnResidentStore *store, const int32_t *slots, int B, int64_t M, int task_space, int64_t total_verts, int64_t max_nf,
                              int kind, int use_clip, float tsdf_clip, int absolute, const float *query, void *ws, size_t ws_bytes, float *value,
                              int64_t *bad, void *stream);
/* M points of the garment mesh per garment: query [B][M][3] from the NOCS vertices and target from the simulation vertices (rot turns the target); task_space
 * != 0: faces by cdf_task, query from task_verts (rot turns it about (0.5, 0.5, 0)), target from the NOCS vertices */
int gn_resident_surface(const GnResidentStore *store, const int32_t *slots, int B, int M, const double *face_u, const double *uv, int task_space,
                        const float *rot, float *query, float *target, void *stream);
/* M points of the marching-cubes mesh per garment: query [B][M][3], on_surf [B][M] = interpolated is_vertex_on_surface > 0.5 as 0 / 1 */
int gn_resident_mc_surface(const GnResidentStore *store, const int32_t *slots, int B, int M, const double *face_u, const double *uv, float *query,
                           float *on_surf, void *stream);

/* ---- Training monitors (csrc/render.hip; DESIGN.md "Training monitors"): the reference's z-buffered point splat (common/rendering_util.py) and its
 * colouring, every image of a batch in one launch each.  No atomics: a pixel is written once by its owner, identical calls give identical bits. ---- */

#define GN_RENDER_MAX_SIZE 4096      /* 1 <= S <= this */
#define GN_RENDER_MAX_OVERLAYS 3
#define GN_RENDER_FRONT 0            /* camera (x, 1 - z, y) */
#define GN_RENDER_TOP 1              /* camera (x, 1 - y, 1 - z) */
#define GN_RENDER_LEFT 2             /* camera (1 - y, 1 - z, x) */
#define GN_COLOR_TABLE 0             /* colour = colors[offset + idx] */
#define GN_COLOR_VIRIDIS 1           /* colour = viridis((values[offset + idx] - vmin) / (vmax - vmin)), matplotlib's Colormap.__call__ in fp32 */

typedef struct {
    float xyz[3], rgba[4];           /* a point in the image's own space (it goes through the image's camera) and its colour; alpha <= 0: not drawn */
    int32_t kernel_size;
} GnOverlayPoint;

typedef struct {
    int64_t offset, count;           /* the image's rows of colors / entries of values; an index >= count keeps the default colour */
    int32_t mode, side;              /* GN_COLOR_*, GN_RENDER_* */
    float vmin, vmax;
    float default_color[4];
    int32_t num_overlays, pad;
    GnOverlayPoint overlay[GN_RENDER_MAX_OVERLAYS];   /* applied in order, each over the ones before */
} GnColorImage;

/* points [N][3] fp32 -> out [I][S][S] uint32: image i draws the points seg[i] .. seg[i+1] from side[i] with a kernel_size[i]-wide footprint; a pixel holds
 * the index (from the start of its image's segment) of the covering point with the smallest camera depth in fp64, the lowest index among equal depths,
 * 0xFFFFFFFF when nobody covers it.  A point with a non-finite coordinate is not drawn.  seg_host [I+1], side_host [I], kernel_size_host [I]: HOST arrays,
 * checked here (S in [1, GN_RENDER_MAX_SIZE], 1 <= k <= S, I <= 65535, a segment shorter than 2^32 - 1, side in {0, 1, 2}); tab [I][4] int64: the same
 * (first point, end point, side, kernel_size) per image in DEVICE memory, what the kernel reads. */
int gn_render_points_batch(const float *points, const int64_t *seg_host, const int32_t *side_host, const int32_t *kernel_size_host, const int64_t *tab,
                           int I, int S, uint32_t *out, void *stream);
/* idx_img [I][S][S] -> out [I][S][S][4] fp32 RGBA: default_color where the index is 0xFFFFFFFF, else the image's colour of that index; then the overlay
 * points, each a one-point image of its own footprint copied where it is drawn (the reference's overlay_grip).  tab_host: the table on the HOST (checked
 * here); tab: the same table in DEVICE memory; colors [..][4] (16-byte aligned) and values [..] fp32, NULL when no image reads them. */
int gn_color_idx_batch(const uint32_t *idx_img, const GnColorImage *tab_host, const GnColorImage *tab, const float *colors, const float *values, int I,
                       int S, float *out, void *stream);

/* ---- Mesh images (csrc/render.hip; DESIGN.md "Mesh images"): a z-buffered, two-sided, shaded triangle rasteriser behind the same camera, every image of
 * a batch in one launch each.  Coverage and ownership of shared edges are decided in integers on 1/256-pixel fixed-point coordinates; no atomics. ---- */

typedef struct {
    int64_t vert_begin, vert_end;    /* the image's rows of verts and of colors; a face indexes from vert_begin */
    int64_t face_begin, face_end;    /* the image's rows of faces; a pixel's index counts from face_begin */
    int32_t side;                    /* GN_RENDER_* */
    float ambient;                   /* shade = ambient + (1 - ambient) * |n_z| / |n|, in [0, 1] */
    float default_color[4];          /* pixels nobody covers */
} GnMeshImage;

/* verts [..][3] fp32, faces [..][3] int32 -> out [I][S][S] uint32: per pixel the index (from face_begin) of the face that covers the pixel's sample with
 * the smallest interpolated camera depth (fp64), the lowest index among equal depths, 0xFFFFFFFF when nobody covers it.  Never drawn: a face with a vertex
 * index outside [0, vert_end - vert_begin), with a non-finite coordinate, with a fixed-point coordinate beyond 2^24 in magnitude, or of zero area.
 * vseg_host, fseg_host [I+1] and tab_host [I]: HOST arrays, checked here (non-decreasing CSRs that the table repeats, fewer than 2^32 - 1 faces per image,
 * side in {0, 1, 2}, ambient in [0, 1], I <= 65535, S in [1, GN_RENDER_MAX_SIZE]); tab: the same table in DEVICE memory, what the kernel reads. */
int gn_render_mesh_batch(const float *verts, const int32_t *faces, const int64_t *vseg_host, const int64_t *fseg_host, const GnMeshImage *tab_host,
                         const GnMeshImage *tab, int I, int S, uint32_t *out, void *stream);
/* idx_img [I][S][S] (gn_render_mesh_batch's, same verts / faces / table) -> out [I][S][S][4] fp32 RGBA: default_color where the index is 0xFFFFFFFF,
 * else shade * the barycentric mix of the face's three rows of colors [..][4] (one row per row of verts), alpha 1. */
int gn_color_mesh_batch(const uint32_t *idx_img, const float *verts, const int32_t *faces, const float *colors, const int64_t *vseg_host,
                        const int64_t *fseg_host, const GnMeshImage *tab_host, const GnMeshImage *tab, int I, int S, float *out, void *stream);

/* ---- Point clouds from meshes (csrc/render.hip; DESIGN.md "Point clouds from meshes"): the same rasteriser behind a free-standing perspective camera,
 * perspective-correct depth and attributes, and the covered pixels compacted into point rows in raster order.  No atomics anywhere. ---- */

typedef struct {
    int64_t vert_begin, vert_end;    /* the rows of verts (and of nocs) of the image's mesh; a face indexes from vert_begin */
    int64_t face_begin, face_end;    /* the rows of faces of the image's mesh; a pixel's index counts from face_begin */
    double R[9], t[3];               /* world -> camera (x right, y down, z forward): cam[j] = ((R[3j] x + R[3j+1] y) + R[3j+2] z) + t[j] */
    double f, c, znear;              /* u = (f * cam[0]) / cam[2] + c, v likewise; a face with a vertex at cam[2] < znear ("near") is never drawn */
    float ambient;                   /* shade = ambient + (1 - ambient) * |n.p| / sqrt((n.n)(p.p)), in [0, 1] */
    float base_color[3];             /* rgb = uint8(clamp(rint(255 * shade * base_color), 0, 255)) */
} GnDepthImage;

/* verts [..][3] fp32, faces [..][3] int32 -> out [I][S][S] uint32: per pixel the index (from face_begin) of the face that covers the pixel's sample with
 * the LARGEST perspective-correct inverse depth (fp64), the lowest index among equal ones, 0xFFFFFFFF when nobody covers it.  Never drawn: what
 * gn_render_mesh_batch never draws, and a face with a vertex at cam[2] < near.  Several images may share a mesh: vseg_host, fseg_host [M+1] are the CSRs of
 * the M meshes and mesh_host [I] names each image's mesh.  HOST arrays, checked here (non-decreasing CSRs that the table repeats through mesh_host, fewer than
 * 2^32 - 1 faces per mesh, finite R and t, f > 0 and finite, c finite, near > 0 and finite, ambient in [0, 1], I <= 65535, S in [1, GN_RENDER_MAX_SIZE]); tab:
 * the same table in DEVICE memory, what the kernels read. */
int gn_depth_render_batch(const float *verts, const int32_t *faces, const int64_t *vseg_host, const int64_t *fseg_host, int M, const int32_t *mesh_host,
                          const GnDepthImage *tab_host, const GnDepthImage *tab, int I, int S, uint32_t *out, void *stream);
/* idx_img [I][S][S] -> row_off [I*S+1] int64: the exclusive prefix sum, over image rows in (image, Y) order, of the number of covered pixels (index !=
 * 0xFFFFFFFF) per row, the total last; sizes [I] int64: covered pixels per image.  A count per row (one wave each), then one scan. */
int gn_depth_cloud_offsets(const uint32_t *idx_img, int I, int S, int64_t *row_off, int64_t *sizes, void *stream);
/* the covered pixels of idx_img (gn_depth_render_batch's, same verts / faces / table) as point rows, image after image, within an image in raster order
 * (Y, then X): the pixel of row offset r writes point [r][3] fp32 (the perspective-correct mix of the face's corners), nocs_out [r][3] fp32 (the same mix
 * of the rows of nocs [..][3], one per row of verts) and rgb [r][3] uint8.  row_off: gn_depth_cloud_offsets' of the same idx_img; N: the rows the three
 * outputs hold (row_off's total); a row offset outside [0, N) is not written. */
int gn_depth_cloud_write(const uint32_t *idx_img, const float *verts, const float *nocs, const int32_t *faces, const int64_t *vseg_host,
                         const int64_t *fseg_host, int M, const int32_t *mesh_host, const GnDepthImage *tab_host, const GnDepthImage *tab,
                         const int64_t *row_off, int I, int S, int64_t N, float *point, float *nocs_out, uint8_t *rgb, void *stream);

/* The hanging garment (garmentnets_amd/cloth.py has the definition, DESIGN.md "Hanging garments"): `substeps` substeps of small-step XPBD on each of B
 * ragged garments, fp64, bit for bit cloth.simulate_reference.  ONE workgroup of `block` threads (a multiple of 64 in [64, 1024]) owns one garment, so the
 * result is a pure function of (garment, constants, substeps): independent of the batch, of `block`, of lds_bytes and of max_substeps_per_launch.
 * x, v [*][3] fp64, in and out (carried in global memory between the launches of one call: at most max_substeps_per_launch substeps per launch);
 * w [*] inverse masses (0: held or massless, never moved); pairs [*][2] int32 vertex indices relative to the garment's first vertex, grouped by colour
 * (no two constraints of a colour share a vertex); l0, alpha_t [*] per constraint.  csr [B + 1][3] int64 on the device = {v_off, c_off, k_off}, closed by
 * the totals: garment b owns the vertex rows v_off[b] .. v_off[b+1] - 1, the constraint rows c_off[b] .. c_off[b+1] - 1 and the entries
 * k_off[b] .. k_off[b+1] - 1 of colour_off (K_b + 1 of them for K_b colours, relative to c_off[b]).  consts_host [6] = {h, 1/h, h*g.x, h*g.y, h*g.z,
 * damp}.  A garment whose positions fit lds_bytes (24 bytes per vertex, at most 160 KiB) keeps them in LDS, any other in its rows of x.  An index of
 * `pairs` outside [0, V_b) sets *bad = 1 (caller zeroes it) and is never dereferenced.  Refused by name: B > 65535, 2^31 or more vertices or
 * constraints in all, a bad block / lds_bytes / substep count, a step constant that is not finite, null pointers. */
int gn_cloth_simulate_batch(double *x, double *v, const double *w, const int32_t *pairs, const double *l0, const double *alpha_t, const int64_t *csr,
                            const int64_t *colour_off, int B, int64_t total_verts, int64_t total_constraints, int64_t substeps,
                            int max_substeps_per_launch, const double *consts_host, int lds_bytes, int block, int64_t *bad, void *stream);

/* Self-collision of the hanging garment (cloth.py "Self-collision"; DESIGN.md "Hanging garments").  The vertex-vertex contact lists of B ragged garments
 * for the positions x [*][3] fp64 and the start poses x0 [*][3], through a uniform grid of cells hashed into `buckets` buckets per garment
 * (gn_cloth_contact_buckets(max_verts) or any larger power of two; max_verts: the most vertices a garment of the batch has) -- bit for bit the
 * brute-force lists of cloth.contact_lists_reference.  csr: the solver's table (only v_off is read).  collision_host [4] = {t2, r2, cell edge (> r),
 * relax}.  flags: 1 = measure the travel against the positions stored at the last build, 2 = build the lists (and store the positions), 3 = both, the
 * travel first.  A build writes, per vertex row, list_j [*][K] (ascending partner indices relative to the garment's first vertex, -1 beyond the row's
 * entries), list_tm2 [*][K] (min(t2, rest2) of the entry, 0 beyond), list_n [*] (entries, at most K) and list_total [*] (the uncut length), and
 * accumulates into diag [B][4] int64 (caller zeroes it once per run) {sum of list_total - list_n, largest list_total, -- (the solver's active entries),
 * the bits of the largest squared travel as a double}.  workspace: gn_cloth_contact_workspace_bytes(total_verts, B, buckets) bytes, kept by the caller
 * between the calls of one run (it holds the stored positions).  Refused by name: B > 65535, 2^31 / 64 or more vertices, K outside [1, 64], bad flags
 * or buckets, a constant that is not finite and positive, a cell edge that does not exceed r, a short workspace, null pointers. */
int gn_cloth_contact_buckets(int max_verts);
size_t gn_cloth_contact_workspace_bytes(int64_t total_verts, int B, int buckets);
int gn_cloth_contact_lists(const double *x, const double *x0, const int64_t *csr, int B, int64_t total_verts, int max_verts, int buckets,
                           const double *collision_host, int K, int flags, void *workspace, size_t workspace_bytes, int32_t *list_j, double *list_tm2,
                           int32_t *list_n, int32_t *list_total, int64_t *diag, void *stream);

/* gn_cloth_simulate_batch with the contact pass of the definition after the last colour of every substep: the lists of gn_cloth_contact_lists (list_j,
 * list_tm2, list_n, rows of stride K), corr [*][3] fp64 workspace, diag as above (diag[b][2] += the active entries).  The caller runs at most the
 * substeps up to the next rebuild per call and alternates the two entries on one stream.  A list index outside [0, V_b) sets *bad and is never
 * dereferenced.  Refused by name, beside gn_cloth_simulate_batch's refusals: K outside [1, 64], relax (collision_host[3]) outside (0, 1], null lists. */
int gn_cloth_simulate_contacts_batch(double *x, double *v, const double *w, const int32_t *pairs, const double *l0, const double *alpha_t,
                                     const int64_t *csr, const int64_t *colour_off, int B, int64_t total_verts, int64_t total_constraints,
                                     int64_t substeps, int max_substeps_per_launch, const double *consts_host, int lds_bytes, int block, int64_t *bad,
                                     const int32_t *list_j, const double *list_tm2, const int32_t *list_n, int K, const double *collision_host,
                                     double *corr, int64_t *diag, void *stream);

/* Vertex-face contacts of the hanging garment (cloth.py "Vertex-face contacts"; DESIGN.md "Hanging garments").  The face-contact lists of B ragged
 * garments for the positions x and the start poses x0, over ALL (vertex, face) pairs -- bit for bit cloth.face_contact_lists_reference.  csr: the
 * solver's table (only v_off is read); faces [*][3] int32 vertex indices relative to the garment's first vertex; fcsr [B + 1] int64 the garments'
 * first faces.  face_host [2] = {tf2, rf2}; collision_host: the vertex contacts' constants (must be given: face contacts need them on; not read
 * further).  `chunks` in [1, 1024] spreads the faces of a garment over that many workgroups per block of 256 vertices (the lists do not depend on
 * it); hit_f / hit_tm2 [total_verts][chunks][Kf] (hit_entries entries each) and hit_n [total_verts][chunks] (hit_rows rows) hold the per-chunk hits
 * between the two kernels.  Written per vertex row: list_f [*][Kf] (ascending face indices relative to the garment's first face, -1 beyond the row's
 * entries), list_tm2 [*][Kf] (min(tf2, the rest squared distance), 0 beyond), list_n [*] (entries, at most Kf), list_total [*] (the uncut length);
 * list_entries / list_rows are the sizes the caller allocated.  fdiag [fdiag_rows >= B][3] int64 (caller zeroes it once per run) accumulates {sum of
 * list_total - list_n, largest list_total, -- (the solver's active face entries)}.  A face index outside [0, V_b) sets *bad (caller zeroes it) and
 * is never dereferenced.  Refused by name: B > 65535, chunks outside [1, 1024], Kf outside [1, 32], a face constant that is not finite and positive,
 * null collision constants, too many vertices / faces, short hit buffers / lists / fdiag, null pointers. */
int gn_cloth_face_contact_lists(const double *x, const double *x0, const int64_t *csr, const int32_t *faces, const int64_t *fcsr, int B,
                                int64_t total_verts, int64_t total_faces, int max_verts, const double *face_host, const double *collision_host, int Kf,
                                int chunks, int32_t *hit_f, double *hit_tm2, int64_t hit_entries, int32_t *hit_n, int64_t hit_rows, int32_t *list_f,
                                double *list_tm2, int64_t list_entries, int32_t *list_n, int32_t *list_total, int64_t list_rows, int64_t *fdiag,
                                int64_t fdiag_rows, int64_t *bad, void *stream);

/* gn_cloth_simulate_contacts_batch with the face entries of the definition inside the same gather: for a vertex its vertex entries first, then its
 * face entries (flist_f, flist_tm2, flist_n: the lists of gn_cloth_face_contact_lists, rows of stride Kf), both into one corr, before the single
 * p += relax * corr.  fdiag[b][2] += the active face entries.  A face-list index outside [0, F_b) or a face corner outside [0, V_b) sets *bad and is
 * never dereferenced.  Refused by name, beside gn_cloth_simulate_contacts_batch's refusals: Kf outside [1, 32], a face constant that is not finite
 * and positive, null collision constants, short face lists / fdiag, null faces / fcsr / lists. */
int gn_cloth_simulate_face_contacts_batch(double *x, double *v, const double *w, const int32_t *pairs, const double *l0, const double *alpha_t,
                                          const int64_t *csr, const int64_t *colour_off, int B, int64_t total_verts, int64_t total_constraints,
                                          int64_t substeps, int max_substeps_per_launch, const double *consts_host, int lds_bytes, int block,
                                          int64_t *bad, const int32_t *list_j, const double *list_tm2, const int32_t *list_n, int K,
                                          const double *collision_host, double *corr, int64_t *diag, const int32_t *faces, const int64_t *fcsr,
                                          int64_t total_faces, const int32_t *flist_f, const double *flist_tm2, int64_t flist_entries,
                                          const int32_t *flist_n, int64_t flist_rows, int Kf, const double *face_host, int64_t *fdiag,
                                          int64_t fdiag_rows, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GARMENTNETS_HIP_H */
