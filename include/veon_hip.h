/*
 * veon_hip.h -- C ABI of libveon_hip.so: the MI355X (gfx950) drop-in for the
 * native half of VEON's Lift-Splat hot path.
 *
 * Conventions (mirroring the reference launchers, which are already plain C
 * functions over raw pointers -- mmdet3d/ops/bev_pool_v2/src/bev_pool.cpp:7-14):
 *   - every pointer is a DEVICE pointer owned by the caller; the library never
 *     allocates, frees or retains memory across calls (workspaces are passed in);
 *   - every launch goes to the `stream` argument (a hipStream_t passed as
 *     void*; NULL = the null stream), is asynchronous and is hipGraph-capturable;
 *   - every entry point returns VEON_OK (0) or a VEON_ERR_* code; nothing is
 *     printed.  The reference returns void and checks nothing;
 *   - index ARRAYS are int32 (the reference ABI); offsets derived from them are
 *     computed in 64 bits (the reference overflows int32 at batch >= 14 with
 *     C = 256: bev_pool_cuda.cu:41,46).
 * Paths below are relative to the reference tree.
 */
/*
 * The ctypes binding (veon_amd/_lib.py) reads its argument types from THIS file, so
 * every declaration below keeps to one style: C89 prototypes `ret veon_name(args);`
 * (they may span lines) with ret in {int, int64_t, void, const char *} and parameters
 * int / int64_t / float / double / unsigned, a pointer (any pointer is passed as an address)
 * or veon_image_windows by value; `(void)` for no parameters; comments are C block
 * comments; the only other statements are the three `typedef struct`s.  Anything else makes the binding raise at import.
 * Prototypes are grouped by the source file under veon_amd/csrc/ that defines them;
 * every entry point that launches work ends in `void *stream`.
 */
#ifndef VEON_HIP_H_
#define VEON_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: veon_vit_block_weights grew the trailing field q_log2 (round 3); every entry point
 * that existed under version 1 keeps its signature and meaning. */
#define VEON_ABI_VERSION 2

#define VEON_OK 0
#define VEON_ERR_BAD_ARG 1    /* null pointer, negative size, unsupported shape */
#define VEON_ERR_LAUNCH 2     /* hipGetLastError() != hipSuccess after launch   */
#define VEON_ERR_WORKSPACE 3  /* workspace too small                            */

/* output layouts of the fused forward */
#define VEON_LAYOUT_BZYXC 0 /* (B,Z,Y,X,C): QuickCumsumCuda's `out`, bev_pool.py:27 */
#define VEON_LAYOUT_BCZYX 1 /* (B,C,Z,Y,X): bev_pool_v2()'s return, bev_pool.py:91  */

/* storage type of the feature rows for the *_ex entry points */
#define VEON_FEAT_F32 0
#define VEON_FEAT_F16 1  /* IEEE half */
#define VEON_FEAT_BF16 2

/* ======== bev_pool_v2.hip =========================================================== */

int veon_abi_version(void);
/* 16-bit operand type this build of the library was compiled for: 0 = bf16
 * (libveon_hip.so), 1 = IEEE fp16 (libveon_hip_f16.so: the same sources with
 * -DVEON_HALF_FP16).  Every entry point named *_bf16 and every "bf16" buffer in
 * this header means "the half type of the build"; accumulation is fp32 in both. */
int veon_half_mode(void);
const char *veon_status_string(int status);

/*
 * Drop-in for `void bev_pool_v2(int c, int n_intervals, ...)`
 * (mmdet3d/ops/bev_pool_v2/src/bev_pool_cuda.cu:125-131, declared
 * bev_pool.cpp:7-9).  Same argument order and meaning; `out` is
 * [n_voxels][c], must be zero-filled by the caller (bev_pool.py:27) and only
 * rows named by ranks_bev[interval_starts[i]] are written.  Any interval
 * order is accepted.  Per (interval, channel) the sum is a serial fmaf chain
 * in storage order, as the reference kernel's (:38-43).
 */
int veon_bev_pool_v2_fwd(int c, int n_intervals, const float *depth,
                         const float *feat, const int *ranks_depth,
                         const int *ranks_feat, const int *ranks_bev,
                         const int *interval_starts,
                         const int *interval_lengths, float *out, void *stream);

/*
 * Drop-in for `void bev_pool_v2_grad(int c, int n_intervals, ...)`
 * (bev_pool_cuda.cu:133-140, declared bev_pool.cpp:11-14).  Intervals are over
 * the ranks_feat-sorted point list (bev_pool.py:47-57).  depth_grad / feat_grad
 * must be zero-filled by the caller (bev_pool.py:67-68); out_grad is
 * [n_voxels][c].
 */
int veon_bev_pool_v2_bwd(int c, int n_intervals, const float *out_grad,
                         const float *depth, const float *feat,
                         const int *ranks_depth, const int *ranks_feat,
                         const int *ranks_bev, const int *interval_starts,
                         const int *interval_lengths, float *depth_grad,
                         float *feat_grad, void *stream);

/*
 * Pool plan for the fused forward.  The fused kernels walk the output in tiles
 * of veon_bev_pool_tile_voxels() consecutive voxel ranks; plan entry t is
 * {first interval, #intervals, first point, #points} of tile t.  `plan` must
 * hold veon_bev_pool_plan_ints(batch, voxels_per_batch) int32 values, 16-byte
 * aligned; the first 4*n_tiles are the entries, the rest is build scratch.
 * Build it once beside the five rank arrays when they are cached (the
 * accelerate=True path, view_transformer_raw.py:196-215), or per call
 * (two tiny kernels).  `counts` (optional DEVICE int[2] = {points, intervals})
 * overrides n_points / n_intervals, which then only bound the launch.
 * Requires the intervals ascending and unique in
 * ranks_bev[interval_starts[i]] -- what voxel_pooling_prepare_v2 produces
 * (view_transformer_raw.py:287-299).
 */
int veon_bev_pool_tile_voxels(void);
int64_t veon_bev_pool_plan_ints(int batch, int64_t voxels_per_batch);
int veon_bev_pool_plan(int n_intervals, int n_points, int batch,
                       int64_t voxels_per_batch, const int *ranks_bev,
                       const int *interval_starts, const int *counts, int *plan,
                       void *stream);

/*
 * Fused forward: zero-fill + pool (+ layout permute) in ONE pass; every
 * element of `out` is written exactly once, so `out` may be uninitialised.
 * Replaces the three full-volume passes of the reference
 * (new_zeros bev_pool.py:27, kernel store bev_pool_cuda.cu:46-47,
 * permute().contiguous() bev_pool.py:91).  Same summation as
 * veon_bev_pool_v2_fwd (serial fmaf chain per interval), so the results are
 * bit-identical to the three-pass structure.
 * Preconditions: as veon_bev_pool_plan; all ranks < batch * voxels_per_batch.
 */
int veon_bev_pool_v2_fwd_fused(int c, int n_intervals, int batch,
                               int64_t voxels_per_batch, const float *depth,
                               const float *feat, const int *ranks_depth,
                               const int *ranks_feat, const int *ranks_bev,
                               const int *interval_starts,
                               const int *interval_lengths, const int *plan,
                               float *out, int out_layout, void *stream);

/*
 * Fused forward + max-pool: LSSViewTransformerRaw.forward's
 * `bev_pool_v2` followed by the (dz,dy,dx) block max
 * (view_transformer_raw.py:545-553) in one kernel; the full-resolution volume
 * is never written.  out is (B, C, Z/dz, Y/dy, X/dx) fp32, every element
 * written.  Bit-equal to max-pooling veon_bev_pool_v2_fwd_fused's output.
 * row_first: veon_bev_pool_row_table(..., row_voxels = X, ...) -- first
 * interval of every (b,z,y) row of X voxels, B*Z*Y+1 entries (row_point, same
 * size, receives the first point of every row).  `counts` (optional DEVICE
 * int[2] = {points, intervals}, e.g. veon_lss_prepare's) overrides
 * n_points / n_intervals, which then only bound the launch (pass the buffer
 * capacity).  Same preconditions as veon_bev_pool_plan.
 */
int veon_bev_pool_row_table(int n_intervals, int n_points, int batch,
                            int64_t voxels_per_batch, int row_voxels,
                            const int *ranks_bev, const int *interval_starts,
                            const int *counts, int *row_first, int *row_point,
                            void *stream);
int veon_bev_pool_v2_fwd_maxpool(int c, int n_intervals, int batch, int Z, int Y,
                                 int X, int dz, int dy, int dx,
                                 const float *depth, const float *feat,
                                 const int *ranks_depth, const int *ranks_feat,
                                 const int *ranks_bev,
                                 const int *interval_starts,
                                 const int *interval_lengths,
                                 const int *row_first, float *out,
                                 void *stream);

/*
 * Half-precision feature rows.  QuickCumsumCuda.forward widens feat to fp32
 * before the kernel (bev_pool.py:21 `feat.contiguous().float()`); the *_ex
 * entry points read fp16 / bf16 rows (`feat_dtype` = VEON_FEAT_*) and widen in
 * registers -- identical arithmetic (the widening is exact, the fmaf chain and
 * the output stay fp32) at half the gather bytes and no fp32 copy of feat.
 * With VEON_FEAT_F32 they are the functions above.
 */
int veon_bev_pool_v2_fwd_fused_ex(int c, int n_intervals, int batch,
                                  int64_t voxels_per_batch, const float *depth,
                                  const void *feat, int feat_dtype,
                                  const int *ranks_depth, const int *ranks_feat,
                                  const int *ranks_bev,
                                  const int *interval_starts,
                                  const int *interval_lengths, const int *plan,
                                  float *out, int out_layout, void *stream);
int veon_bev_pool_v2_fwd_maxpool_ex(int c, int n_intervals, int batch, int Z,
                                    int Y, int X, int dz, int dy, int dx,
                                    const float *depth, const void *feat,
                                    int feat_dtype, const int *ranks_depth,
                                    const int *ranks_feat, const int *ranks_bev,
                                    const int *interval_starts,
                                    const int *interval_lengths,
                                    const int *row_first, float *out,
                                    void *stream);

/* As veon_bev_pool_v2_fwd_fused_ex with the (B,C,Z,Y,X) layout, but the channel
 * planes of `out` are `plane_stride` floats apart (>= voxels_per_batch): out is a
 * (B, C, plane_stride) buffer whose first voxels_per_batch floats of every plane
 * are written.  For consumers that take a strided view, and for
 * tools/stride_probe.py (placement sensitivity of the plane streams). */
int veon_bev_pool_v2_fwd_fused_strided(int c, int n_intervals, int batch,
                                       int64_t voxels_per_batch, const float *depth,
                                       const void *feat, int feat_dtype,
                                       const int *ranks_depth, const int *ranks_feat,
                                       const int *ranks_bev,
                                       const int *interval_starts,
                                       const int *interval_lengths, const int *plan,
                                       float *out, int64_t plane_stride,
                                       void *stream);

/* (images, C, HW) -> (images, HW, C), 4- or 2-byte elements: the
 * `feat.permute(0, 1, 3, 4, 2)` of view_transform_core (view_transformer.py:273-275)
 * made contiguous, as bev_pool_v2 does on entry (bev_pool.py:21). */
int veon_feat_nchw_to_nhwc(const void *in, void *out, int elem_bytes, int images,
                           int C, int HW, void *stream);

/*
 * The fused pool + max-pool writing straight into the Conv3d body's input: the
 * interior of the zero-padded channels-last bf16 grid [B][Z/dz+2][Y/dy+2][X/dx+2][C]
 * (see veon_conv3d_k3_bf16; allocate it zeroed once, the halo is never
 * written).  Values are the fp32 results of veon_bev_pool_v2_fwd_maxpool_ex
 * rounded to bf16 -- what veon_volume_pack_bf16 of that tensor would store.
 */
int veon_bev_pool_v2_fwd_maxpool_padded(int c, int n_intervals, int batch, int Z,
                                        int Y, int X, int dz, int dy, int dx,
                                        const float *depth, const void *feat,
                                        int feat_dtype, const int *ranks_depth,
                                        const int *ranks_feat,
                                        const int *ranks_bev,
                                        const int *interval_starts,
                                        const int *interval_lengths,
                                        const int *row_first,
                                        void *out_padded_bf16, void *stream);

/*
 * 2x2x2 block max of a (B,C,Z,Y,X) fp32 volume -> (B,C,Z/2,Y/2,X/2) fp32: the
 * ds_feat step of LSSViewTransformerRaw.forward (view_transformer_raw.py:549-553:
 * rearrange + max over the three block axes) as one streaming pass, for volumes that
 * did not come out of the fused pool + max-pool kernel (the camera-sharded path: the
 * block max follows the cross-rank sum).  planes = B * C; Z, Y, X even.  NaN
 * propagates as in torch.amax.
 */
int veon_volume_maxpool2_f32(const float *in, float *out, int64_t planes, int Z, int Y,
                             int X, void *stream);

/* ======== bev_pool_rows.hip ========================================================= */

/*
 * ---- "row" kernels: the wide-channel shapes (VEON: C = 256) ----------------
 * Same arithmetic as the fused entry points above (serial fmaf chain per voxel
 * in storage order, bev_pool_cuda.cu:38-43), different decomposition: the index
 * side is ONE dense table
 *     vstart[B*voxels_per_batch + 1]:  voxel v owns points
 *     [vstart[v], vstart[v+1]) of the rank-sorted arrays
 * (the exclusive scan of the voxel histogram -- veon_lss_prepare emits it as
 * `vstart`; veon_bev_pool_voxel_table builds it from the reference's arrays
 * ranks_bev / interval_starts, which must be ascending in voxel rank and tile
 * the point arrays, i.e. starts[i+1] == starts[i] + lengths[i] -- what
 * voxel_pooling_prepare_v2 produces, view_transformer_raw.py:287-299); the
 * gather side reads every feature row once per workgroup as one full-width wave
 * load (lanes = channels).  ranks_bev / interval_* are not read by the kernels.
 *
 * veon_bev_pool_v2_fwd_rows: zero-fill + pool + (B,C,Z,Y,X) layout in one pass
 *   (as veon_bev_pool_v2_fwd_fused_strided; plane_stride 0 = contiguous).
 *   c even.  `variant` selects the tile shape (0 = default).
 * veon_bev_pool_v2_fwd_rows_maxpool: pool + (2,2,2) block max
 *   (LSSViewTransformerRaw.forward, view_transformer_raw.py:545-553).
 *   out_padded_bf16 = 0: out is (B,C,Z/2,Y/2,X/2) fp32;  1: out is the interior
 *   of the Conv3d body's zero-padded channels-last bf16 grid (as
 *   veon_bev_pool_v2_fwd_maxpool_padded).  c % 4 == 0.
 * feat_elems: number of elements of `feat` (rows * c); must be < 2^31 (row offsets
 *   are 32-bit inside the kernels; every ranks_feat value must be a valid row).
 */
int64_t veon_bev_pool_voxel_table_ints(int batch, int64_t voxels_per_batch);
int veon_bev_pool_voxel_table(int n_intervals, int n_points, int batch,
                              int64_t voxels_per_batch, const int *ranks_bev,
                              const int *interval_starts, const int *counts,
                              int *vstart, void *stream);
int veon_bev_pool_v2_fwd_rows(int c, int batch, int64_t voxels_per_batch,
                              const float *depth, const void *feat, int feat_dtype,
                              const int *ranks_depth, const int *ranks_feat,
                              const int *vstart, float *out, int64_t plane_stride,
                              int64_t feat_elems, int variant, void *stream);
int veon_bev_pool_v2_fwd_rows_maxpool(int c, int batch, int Z, int Y, int X, int dz,
                                      int dy, int dx, const float *depth,
                                      const void *feat, int feat_dtype,
                                      const int *ranks_depth, const int *ranks_feat,
                                      const int *vstart, void *out, int out_padded_bf16,
                                      int64_t feat_elems, void *stream);

/*
 * The same with a caller-given order of the short-list ("cold") work: the pooled
 * volume is cut into chunks of veon_bev_pool_rows_maxpool_chunk() consecutive pooled
 * voxels per batch element (linear (zo, yo, xo) order, chunk id = b * chunks_per_batch
 * + index), cold workgroup i processes chunk chunk_order[i]; chunk_order must be a
 * permutation of all B * ceil(plane / chunk) chunk ids (NULL = built-in order).  Pure
 * scheduling: results never depend on it.  Workgroups are dealt to the eight XCDs
 * round-robin, so an order that gives every XCD the chunks of one azimuth sector around
 * the rig keeps the feature rows of that sector's cameras in the XCD's own 4 MiB L2
 * (veon_amd/ops/bev_pool_v2/bev_pool.py `cold_chunk_order`).
 */
int veon_bev_pool_rows_maxpool_chunk(void);
int veon_bev_pool_v2_fwd_rows_maxpool_ordered(
    int c, int batch, int Z, int Y, int X, int dz, int dy, int dx, const float *depth,
    const void *feat, int feat_dtype, const int *ranks_depth, const int *ranks_feat,
    const int *vstart, void *out, int out_padded_bf16, int64_t feat_elems,
    const int *chunk_order, void *stream);

/*
 * ---- differentiable pool + (2,2,2) block max (training through
 * LSSViewTransformerRaw.forward, view_transformer_raw.py:537-555, with the backward
 * of QuickCumsumCuda, bev_pool.py:43-83, folded in) -- neither direction writes the
 * un-pooled volume.
 *
 * veon_bev_pool_v2_fwd_rows_maxpool_winner: veon_bev_pool_v2_fwd_rows_maxpool_ordered
 *   with fp32 rows (feat_dtype must be VEON_FEAT_F32) and the fp32 (B,C,Z/2,Y/2,X/2)
 *   output, bit-equal to it, plus `winner` (B,Z/2,Y/2,X/2,C) uint8: the smallest child
 *   k = (rz*2 + ry)*2 + rx (the '(dz dh dw)' order of view_transformer_raw.py:549-553)
 *   whose sum equals the block maximum -- the element torch.max(dim=-1) sends the
 *   gradient to -- or 255 when that child holds no point (its zero wins: the
 *   gradient goes nowhere).  4-byte aligned.
 * veon_bev_pool_point_table: pvox[table_len], table_len = B*N*D*H*W: pvox[ranks_depth[p]]
 *   = ranks_bev[p] for every kept point p, -1 elsewhere.  Needs the lift's layout:
 *   every kept point has its own ranks_depth (view_transformer_raw.py:268-270).
 *   Points whose ranks_depth / ranks_bev lie outside [0, table_len) / [0, n_voxels)
 *   are ignored.  `counts` as in veon_bev_pool_voxel_table (n_points then bounds it).
 * veon_bev_pool_v2_bwd_rows_maxpool: with m[p,c] = pooled_grad[q(p),c] if
 *   winner[q(p),c] == child(p) else 0 for the kept points p (q = pooled parent),
 *     depth_grad[ranks_depth[p]] = sum_c m[p,c] * feat[ranks_feat[p],c]
 *     feat_grad[r,c] = sum over the points of pixel r, ascending d, of m[p,c] * depth[..]
 *   for ranks_feat = img*HW + hw, ranks_depth = (img*D + d)*HW + hw
 *   (view_transformer_raw.py:268-274); n_images = B*N.  pooled_grad is channels-last
 *   (B,Z/2,Y/2,X/2,C) fp32.  feat_grad (n_images*HW, c) is written everywhere;
 *   depth_grad must be zero-filled by the caller (as for veon_bev_pool_v2_bwd) and may
 *   be NULL (not computed).  No atomics: results are bit-reproducible.  c % 4 == 0.
 */
int veon_bev_pool_v2_fwd_rows_maxpool_winner(
    int c, int batch, int Z, int Y, int X, int dz, int dy, int dx, const float *depth,
    const void *feat, int feat_dtype, const int *ranks_depth, const int *ranks_feat,
    const int *vstart, void *out, int64_t feat_elems, const int *chunk_order,
    uint8_t *winner, void *stream);
int veon_bev_pool_point_table(int n_points, int64_t table_len, int64_t n_voxels,
                              const int *ranks_depth, const int *ranks_bev,
                              const int *counts, int *pvox, void *stream);
int veon_bev_pool_v2_bwd_rows_maxpool(int c, int n_images, int D, int HW, int batch, int Z,
                                      int Y, int X, const float *pooled_grad,
                                      const uint8_t *winner, const int *pvox,
                                      const float *depth, const float *feat,
                                      float *depth_grad, float *feat_grad, void *stream);

/* ======== lss_prepare.hip =========================================================== */

/*
 * The per-camera 3x3 algebra of get_lidar_coor
 * (view_transformer_raw.py:145,151): post_rots_inv = inv(post_rots),
 * combine = sensor2ego[:3,:3] @ inv(cam2imgs), trans = sensor2ego[:3,3], for BN
 * cameras (sensor2ego (BN,4,4), the others (BN,3,3)).  Stream-capturable
 * replacement for the reference's two torch.inverse calls: adjugate inverse in
 * double precision rounded to float (agrees with LAPACK / rocSOLVER to their
 * own rounding error).
 */
int veon_camera_matrices(int BN, const float *sensor2ego, const float *cam2imgs,
                         const float *post_rots, float *post_rots_inv,
                         float *combine, float *trans, void *stream);

/*
 * Frustum -> ego coordinates: the per-point half of get_lidar_coor
 * (mmdet3d/models/necks/view_transformer_raw.py:144-155).  xs[W], ys[H], ds[D]
 * are the frustum axes (create_frustum, :91-119); post_rots_inv = inv(post_rots)
 * and combine = sensor2ego[:3,:3] @ inv(cam2imgs) are (B,N,3,3), post_trans /
 * trans (B,N,3), bda (B,3,3).  coor is (B,N,D,H,W,3).  Bit-identical to the
 * reference's CPU result for identical matrices.
 */
int veon_lidar_coor(int B, int N, int D, int H, int W, const float *xs,
                    const float *ys, const float *ds,
                    const float *post_rots_inv, const float *post_trans,
                    const float *combine, const float *trans, const float *bda,
                    float *coor, void *stream);

/*
 * voxel_pooling_prepare_v2 (view_transformer_raw.py:244-302) as a counting
 * sort on the device, no host synchronisation inside.
 *   coor != NULL : voxelise the given (B,N,D,H,W,3) coordinates (the method's
 *                  own contract);
 *   coor == NULL : fuse the geometry of veon_lidar_coor in, never
 *                  materialising the coordinates.
 * grid_lower / grid_interval / grid_size are HOST float[3] (the reference's
 * float32 grid tensors, :74-89).  Outputs must hold B*N*D*H*W int32 each; the
 * first counts[0] (points kept) / counts[1] (intervals) entries are valid,
 * counts is DEVICE int[2].  Order inside an interval is ascending ranks_depth
 * (the reference's unstable argsort leaves it unspecified).  A point with a
 * non-finite coordinate (NaN, +-inf -- e.g. every point of a camera whose intrinsic
 * or post_rots matrix is singular) is dropped, like a point outside the grid; the
 * same holds for every veon_lss_prepare_cameras* entry.  `plan` (optional,
 * veon_bev_pool_plan_ints(B, voxels_per_batch) int32, 16-B aligned; needs
 * voxels_per_batch % 64 == 0) receives the fused pool kernels' plan for free.
 * workspace: veon_lss_prepare_workspace_bytes(B*N*D*H*W, B*voxels_per_batch).
 */
int64_t veon_lss_prepare_workspace_bytes(int64_t num_points,
                                         int64_t num_voxels_total);
int veon_lss_prepare(int B, int N, int D, int H, int W, const float *coor,
                     const float *xs, const float *ys, const float *ds,
                     const float *post_rots_inv, const float *post_trans,
                     const float *combine, const float *trans, const float *bda,
                     const float *grid_lower, const float *grid_interval,
                     const float *grid_size, int64_t voxels_per_batch,
                     void *workspace, int64_t workspace_bytes, int *ranks_bev,
                     int *ranks_depth, int *ranks_feat, int *interval_starts,
                     int *interval_lengths, int *plan, int *counts,
                     void *stream);

/*
 * The same prepare straight from the reference's per-camera tensors
 * (get_lidar_coor's arguments, view_transformer_raw.py:121-158: sensor2ego
 * (B,N,4,4), cam2imgs / post_rots (B,N,3,3), post_trans (B,N,3), bda (B,3,3)): the
 * camera algebra of veon_camera_matrices runs inside the first kernel (one launch
 * less, same arithmetic), five launches in all.  Extras for a steady-state,
 * hipGraph-captured caller:
 *   vstart (optional, B*voxels_per_batch + 1 int32): the dense voxel table of the
 *     row pool kernels (veon_bev_pool_voxel_table's output) -- it is the counting
 *     sort's own scan, so it costs nothing;
 *   hist_is_zero = 1: the caller zeroed the WHOLE workspace once (at allocation)
 *     and has only used it for completed calls of this function since: every
 *     call leaves the histogram zeroed again, so no memset node is needed.
 *     With 0 the histogram is cleared first (hipMemsetAsync).
 */
int veon_lss_prepare_cameras(int B, int N, int D, int H, int W, const float *xs,
                             const float *ys, const float *ds,
                             const float *sensor2ego, const float *cam2imgs,
                             const float *post_rots, const float *post_trans,
                             const float *bda, const float *grid_lower,
                             const float *grid_interval, const float *grid_size,
                             int64_t voxels_per_batch, void *workspace,
                             int64_t workspace_bytes, int hist_is_zero,
                             int *ranks_bev, int *ranks_depth, int *ranks_feat,
                             int *interval_starts, int *interval_lengths, int *plan,
                             int *vstart, int *counts, void *stream);

/*
 * Sparse lift (opt-in): the same prepare, but a frustum point whose
 * depth weight depth_weights[(b,n,d,h,w)] (the (B,N,D,H,W) tensor the pool will
 * multiply by) is below depth_eps is dropped before the sort.  VEON's depth is a soft
 * two-hot distribution (view_transformer_raw.py:406-429: softmax of -4|d - c_k|
 * clamped at -16), so all but a handful of the D bins of a pixel carry ~1e-7 of the
 * mass: with depth_eps = 1e-6 the sort, the rank pass and the pool see ~20x fewer
 * points and every pooled sum moves by at most depth_eps * sum|feat| of the dropped
 * points (rtol ~1e-5, the reference's own fp32 reassociation noise).
 * depth_eps = 0 keeps every point (weights are >= 0).
 */
int veon_lss_prepare_cameras_sparse(
    int B, int N, int D, int H, int W, const float *xs, const float *ys, const float *ds,
    const float *sensor2ego, const float *cam2imgs, const float *post_rots,
    const float *post_trans, const float *bda, const float *grid_lower,
    const float *grid_interval, const float *grid_size, int64_t voxels_per_batch,
    void *workspace, int64_t workspace_bytes, int hist_is_zero, int *ranks_bev,
    int *ranks_depth, int *ranks_feat, int *interval_starts, int *interval_lengths,
    int *plan, int *vstart, int *counts, const float *depth_weights, float depth_eps,
    void *stream);

/*
 * Two-hot lift by construction (view_transformer_raw.py:406-429 +
 * 244-302 in one): the same prepare driven by veon_two_hot_window's per-pixel windows
 * instead of a (B,N,D,H,W) weight tensor.  Point (pixel, bin k) is kept iff k lies in
 * the pixel's kept window [q0, q0+nq), or the pixel's tail weight passed the threshold
 * and k lies outside its unclamped window [k0, k0+nk).  ranks_depth then indexes the
 * COMPACT weight table: pix*window_slots + (k in [k0,k0+nk) ? 1 + k - k0 : 0), so every
 * pool entry point of this header is called with depth = wts and computes the sums of
 * the dense lift over the kept points, in the dense lift's order (ascending point
 * index inside a voxel).  With eps = 0 in veon_two_hot_window that is the dense lift
 * to the bit; with eps > 0 every pooled sum moves by at most eps * sum|feat| over the
 * dropped points of its voxel.  ranks_feat / ranks_bev / intervals / vstart / plan /
 * counts as veon_lss_prepare_cameras.
 */
int veon_lss_prepare_cameras_twohot(
    int B, int N, int D, int H, int W, const float *xs, const float *ys, const float *ds,
    const float *sensor2ego, const float *cam2imgs, const float *post_rots,
    const float *post_trans, const float *bda, const float *grid_lower,
    const float *grid_interval, const float *grid_size, int64_t voxels_per_batch,
    void *workspace, int64_t workspace_bytes, int hist_is_zero, int *ranks_bev,
    int *ranks_depth, int *ranks_feat, int *interval_starts, int *interval_lengths,
    int *plan, int *vstart, int *counts, const int *win, int window_slots, void *stream);

/*
 * AlignNetOcc3D.prepare_meta (align_net_occ3d.py:328-352) for one frame: out[b,n] =
 * inverse(ego2global[b,0]) @ ego2global[b,n] @ sensor2ego[b,n], (B,N,4,4) fp32 in and
 * out, the algebra in double precision (the reference casts to double, too).
 */
int veon_sensor2keyego(int B, int N, const float *sensor2ego, const float *ego2global,
                       float *out, void *stream);

/* ======== depth_ops.hip ============================================================= */

/*
 * Depth preparation (LSSViewTransformerRaw.downsample_depth /
 * get_two_hot_depth, view_transformer_raw.py:393-429).
 * veon_downsample_depth: depths (BN,H,W) -> out (BN,H/ds,W/ds), min over the
 *   non-zero pixels of each block (zeros count as 1e5).
 * veon_two_hot_depth: out (BN,D,H,W) = softmax over the D+1 bin centres
 *   c_k = k*step + (lo + step/2) of -gamma*|d - c_k| clamped at -16, last bin
 *   dropped.  ds == 0: depths is (BN,H,W); ds > 0: depths is (BN,H*ds,W*ds) and
 *   the block-min is fused in (the two calls of AlignNetOcc3D.prepare_depth,
 *   align_net_occ3d.py:320-326, in one pass).
 */
int veon_downsample_depth(int BN, int H, int W, int ds, const float *depths,
                          float *out, void *stream);
int veon_two_hot_depth(int BN, int H, int W, int ds, int D, float lo, float step,
                       float gamma, const float *depths, float *out,
                       void *stream);

/*
 * The same distribution in its compact, EXACT form (the
 * (BN,D,H,W) tensor is never written).  A pixel's D+1 logits are -gamma*|d - c_k|
 * where that is >= -16 and exactly -16 elsewhere (view_transformer_raw.py:419-421), so
 * its weights take distinct values only on the contiguous window of unclamped bins
 * [k0, k0+nk) and ONE value -- the tail exp(-16 - max)/sum -- on every other bin.
 *   veon_two_hot_window_slots(D, step, gamma) -> K = 1 + max window length
 *     (floor(32/(gamma*step)) + 2, capped at D); 0 on bad arguments.
 *   wts[pix*K + 0] = tail, wts[pix*K + 1 + j] = weight of bin k0 + j (0 beyond nk);
 *     bit-identical to veon_two_hot_depth's values of those bins.
 *   win[2*pix]     = k0 | nk << 16            unclamped window (bins < D)
 *   win[2*pix + 1] = q0 | nq << 16 | t << 31  [q0, q0+nq): the window bins whose
 *     weight is >= eps (contiguous: the weights are unimodal); t = tail >= eps.
 * depths / ds as veon_two_hot_depth (ds > 0 fuses the block-min).  pix runs over
 * (BN, H, W).  eps = 0 keeps every bin.  win must be 8-byte aligned.
 * Consumed by veon_lss_prepare_cameras_twohot; the pool kernels then take `wts` as
 * their depth table.
 */
int veon_two_hot_window_slots(int D, float step, float gamma);
int veon_two_hot_window(int BN, int H, int W, int ds, int D, float lo, float step,
                        float gamma, float eps, int K, const float *depths, int *win,
                        float *wts, void *stream);

/* ======== vit_block.hip ============================================================= */

/*
 * ViT encoder block kernels (bf16 operands on MFMA, fp32 accumulate, fp32
 * residual stream): the dense contractions of the DINOv2 blocks of
 * DepthAnythingV2 (mmdet3d/models/depth_anything/dinov2_layers/block.py:85-110,
 * attention.py:56-69, mlp.py:40-46, layer_scale.py:27) and of the CLIP
 * residual-attention blocks (semantic_net/clip_utils/visual.py:57-91,
 * attn_helper.py:303-314).  bf16 buffers are passed as void* (uint16 storage).
 *
 * veon_vit_cast_bf16 : fp32 -> bf16 (round to nearest even), n elements.
 * veon_vit_layernorm : x fp32 [T,d] -> bf16 [T,d]; nn.LayerNorm semantics
 *                      (biased variance, eps inside the sqrt), d <= 2048.
 * veon_vit_gemm      : C[M,N] = A[M,K] . W[N,K]^T (+ bias[N]); W is the
 *                      nn.Linear weight layout.  K % 64 == 0, N % 4 == 0.
 *                      epilogue 0: -> bf16 out;  1: GELU(erf) -> bf16 out;
 *                      2: QuickGELU x*sigmoid(1.702x) -> bf16 out;
 *                      3: resid[M,N] (fp32, in place) += gamma[N] * C
 *                         (gamma NULL = 1): LayerScale + residual add.
 *                      4: A.W^T * gamma[N] + bias[N] -> bf16 out (a 1x1x1
 *                         convolution + eval-mode BatchNorm);  5: the same + ReLU
 *                         (the ConvModules of PredHead3DOcc / PredHead3DSem,
 *                         align_net_occ3d.py:431-534);  6: sigmoid(4) - 0.5 (the
 *                         output activation of PredHead3DSem, :528-533).
 * veon_vit_attention : qkv bf16 [B,T,3,H,64] (q pre-scaled) -> out bf16
 *                      [B,T,H*64] = softmax(q k^T + bias) v, flash style.
 *                      bias (optional) fp32 [.,.,T,T] with batch / head strides
 *                      in elements (0 = broadcast).  head_dim must be 64.
 *                      Masking: bias -inf on a key removes it; a query whose keys
 *                      are ALL masked gets an output row of 0 (torch's softmax
 *                      gives NaN there).  Any pattern of masked 64-key tiles is
 *                      exact, however far below zero the live scores lie.
 */
int veon_vit_cast_bf16(const float *in, void *out_bf16, int64_t n, void *stream);
int veon_vit_layernorm(const float *x, const float *gamma, const float *beta,
                       void *out_bf16, int T, int d, float eps, void *stream);
int veon_vit_gemm(const void *a_bf16, const void *w_bf16, const float *bias,
                  const float *gamma, float *resid, void *out_bf16, int M, int N,
                  int K, int epilogue, void *stream);
int veon_vit_attention(const void *qkv_bf16, const float *bias,
                       int64_t bias_batch_stride, int64_t bias_head_stride,
                       void *out_bf16, int B, int T, int H, int head_dim,
                       void *stream);
/* The same with q ALSO multiplied by log2(e) (folded into the projection weights next
 * to head_dim^-0.5): the scores arrive in the exp2 domain and the kernel spends no
 * instruction on scaling them (the form veon_vit_block uses when
 * veon_vit_block_weights.q_log2 is set).  bias stays in natural-log units. */
int veon_vit_attention_log2(const void *qkv_bf16, const float *bias,
                            int64_t bias_batch_stride, int64_t bias_head_stride,
                            void *out_bf16, int B, int T, int H, int head_dim,
                            void *stream);

/* Patch embedding (dinov2_layers/patch_embed.py: Conv2d(kernel = stride = patch)) as a
 * GEMM operand: img fp32 (B,C,H,W) -> bf16 rows [B*(skip + h*w)][kpad], row element
 * c*patch*patch + i*patch + j (the conv weight's order), zero beyond C*patch*patch,
 * ``skip`` zero rows in front of every image (class-token slot).  A remainder of H/W
 * modulo patch is not read (as the convolution). */
int veon_vit_patchify(const float *img, void *out_bf16, int B, int C, int H, int W,
                      int patch, int skip, int kpad, void *stream);

/*
 * Split-K form of the residual GEMM (resid += gamma * (a @ w^T + bias)) for fc2-shaped
 * problems (long K, few output columns: M = 5406, N = 768 / 1024, K = 3072 / 4096): two
 * workgroups per output tile take half of K each, the first to finish parks its fp32
 * accumulators in `slab`, the second adds them to its own and runs the epilogue
 * (deterministic: a + b is commutative).  veon_vit_gemm_splitk_plan -> slab bytes needed
 * (0: the shape is not split).  sync_words (2 ints per tile): ZERO on entry, left zero.
 * veon_vit_block uses it for fc2 with its (by then free) qkv buffer as the slab; the
 * block workspace therefore has to be ZERO when first used (it ends in the sync words).
 */
int64_t veon_vit_gemm_splitk_plan(int M, int N, int K, int *tile_out);
int veon_vit_gemm_splitk(const void *a_bf16, const void *w_bf16, const float *bias,
                         const float *gamma, float *resid, int M, int N, int K,
                         void *slab, int64_t slab_bytes, int *sync_words,
                         int64_t sync_ints, void *stream);

/*
 * One whole pre-norm transformer block on the fp32 residual stream x [B*T, d]
 * (in place): x += g1*(proj(attn(LN1(x)))), x += g2*(fc2(act(fc1(LN2(x))))) --
 * the DINOv2 block (dinov2_layers/block.py:85-110; g = LayerScale) and the CLIP
 * ResidualAttentionBlock (g = NULL, act = QuickGELU).  Seven launches behind
 * one call, so an eager host pays one call per block instead of seven.
 * Weights: bf16 [out,in] row-major with q pre-scaled, fp32 vectors; gamma1/2
 * may be NULL.  act = 1 (GELU erf) or 2 (QuickGELU) -- the veon_vit_gemm
 * epilogue codes.  workspace: veon_vit_block_workspace_bytes(), 256-B aligned.
 */
typedef struct veon_vit_block_weights {
  const float *ln1_w, *ln1_b;
  const void *w_qkv;
  const float *b_qkv;
  const void *w_proj;
  const float *b_proj, *gamma1;
  const float *ln2_w, *ln2_b;
  const void *w_fc1;
  const float *b_fc1;
  const void *w_fc2;
  const float *b_fc2, *gamma2;
  float ln1_eps, ln2_eps;
  int mlp_dim, act;
  int q_log2;   /* 1: w_qkv / b_qkv's q rows carry head_dim^-0.5 * log2(e) (attention in
                   the exp2 domain, veon_vit_attention_log2); 0: head_dim^-0.5 only */
} veon_vit_block_weights;
int64_t veon_vit_block_workspace_bytes(int B, int T, int d, int mlp_dim);
int veon_vit_block(float *x, const veon_vit_block_weights *w,
                   const float *attn_bias, int64_t bias_batch_stride,
                   int64_t bias_head_stride, void *workspace,
                   int64_t workspace_bytes, int B, int T, int d, int H,
                   void *stream);

/*
 * LayerNorm of PADDED rows: x fp32 [T, ld], the token is the first d columns (the rest
 * is padding up to the multiples of 64 the GEMM kernels need); statistics over d,
 * out bf16 [T, ld] with zeros in the padding.  For transformer widths that are not a
 * multiple of 64 -- SAN's side-adapter ViT, width 240 / head_dim 40
 * (side_adaptor_in_veon.py:194-241, timm_wrapper.py:67-74): its blocks run on the
 * kernels above with the width padded to 256 and every head to 64 (zero weight rows /
 * columns, q scaled by 40^-0.5 as before).
 */
int veon_vit_layernorm_padded(const float *x, const float *gamma, const float *beta,
                              void *out_bf16, int T, int d, int ld, float eps,
                              void *stream);

/* nn.LayerNorm over the last dim, fp32 in -> fp32 out, rows of d floats
 * (d % 128 == 0, d <= 1024; this entry point alone also d = 64): the token LayerNorms
 * (ln_3 / ln_4 / pre_norm) of the HSA network's blocks (highres_side_adaptor.py:108-135,
 * 138-193). */
int veon_layernorm_f32(const float *x, const float *gamma, const float *beta,
                       float *out, int T, int d, float eps, void *stream);
/* LayerNorm(x + offset) of (B, L, d) fp32 tokens, where offset is the nearest-neighbour
 * resize (F.interpolate default mode: src = min(floor(dst * in / out), in - 1), the scale
 * in fp32) of a coarser map `add` [B][h*w][d] fp32 to the Y x X token map, added to the
 * LAST Y*X tokens of every sample: the tail of HighresSideAdaptorBlock.forward
 * (highres_side_adaptor.py:123-135 -- neck_add, interpolate, cat / add, ln_4) in one
 * pass instead of upsample + add + cat + LayerNorm. */
int veon_layernorm_f32_add_nearest(const float *x, const float *add, const float *gamma,
                                   const float *beta, float *out, int B, int L, int d,
                                   int Y, int X, int h, int w, float eps, void *stream);
/* the same LayerNorm of (B, Y*X, d) fp32 tokens, written as bf16 into the interior
 * of a zero-haloed channels-last image [B][Y+2][X+2][d] (halo untouched): ln_3
 * followed by the ConvBlock's permute / reshape to a feature map (:113-122, :38-40). */
int veon_layernorm_f32_to_padded(const float *x, const float *gamma, const float *beta,
                                 void *out_padded, int B, int Y, int X, int d,
                                 float eps, void *stream);

/* ======== conv3d.hip ================================================================ */

/*
 * ---- 3x3x3 Conv3d body of the 3D alignment network ----
 * Replaces the Conv3d + BN3d (+ReLU, + identity) of ResBlock3D
 * (mmdet3d/models/semantic_net/side_adapter/align_net_occ3d.py:363-399), which
 * the reference runs as mmcv ConvModules on cuDNN, by an implicit-GEMM MFMA
 * kernel.  Volumes are channels-last bf16 in a zero-padded grid
 * [B][Z+2][Y+2][X+2][C]; `*_padded` pointers address padded voxel (b=0,0,0,0)
 * and the caller must keep veon_conv3d_guard_rows(Y, X) rows of C readable,
 * finite bf16 values before that address and after the last padded row (the
 * kernel reads them for halo outputs, which it then writes as zeros; it never
 * writes guard rows).  w: [Cout][3][3][3][Cin] bf16 (torch's
 * weight.permute(0,2,3,4,1)).  y = conv(in)*scale[n] + shift[n] (eval-mode
 * BatchNorm folded by the caller; either may be NULL), + resid (optional,
 * padded layout, Cout channels), then `relu` = 0 nothing / 1 ReLU / 2 GELU (erf);
 * halo rows of `out` are written
 * as zeros so `out` is a valid padded input of the next conv.  Cin % 64 == 0,
 * Cout % 8 == 0.  out must not alias in.
 */
int64_t veon_conv3d_guard_rows(int Y, int X);
int veon_conv3d_k3_bf16(const void *in_padded, const void *w_bf16,
                        const float *scale, const float *shift,
                        const void *resid_padded, void *out_padded, int B, int Z,
                        int Y, int X, int Cin, int Cout, int relu, void *stream);

/*
 * The 2-D case: 3x3 stride-1 pad-1 convolution on images in the padded
 * channels-last bf16 grid [B][Y+2][X+2][C] (no z halo), same kernel with 9 taps,
 * same epilogue, same guard-row contract.  w: [Cout][3][3][Cin] bf16.  Used for
 * the 3x3 convolutions of DepthAnythingV2's DPT head
 * (mmdet3d/models/depth_anything/dpt.py:39-150, util/blocks.py) when the head
 * runs in bf16.
 */
int veon_conv2d_k3_bf16(const void *in_padded, const void *w_bf16,
                        const float *scale, const float *shift,
                        const void *resid_padded, void *out_padded, int B, int Y,
                        int X, int Cin, int Cout, int relu, void *stream);

/* The same with two optional extras of the epilogue (NULL = absent): a SECOND residual
 * image resid2 (added before the activation) and a second output out_relu that receives
 * relu(result) (not `out_padded` itself).  FeatureFusionBlock (util/blocks.py:86-148)
 * computes  x0 + RCU1(x1)  and every ResidualConvUnit starts with relu(input) (:49-83):
 * with these, conv2 of RCU1 writes x0 + conv + x1 and its ReLU in one pass, and the
 * layer*_rn convolutions write the ReLU of their output next to it -- no elementwise
 * add_ / clamp_min passes over the images. */
int veon_conv2d_k3_bf16_ex(const void *in_padded, const void *w_bf16, const float *scale,
                           const float *shift, const void *resid_padded,
                           const void *resid2_padded, void *out_padded,
                           void *out_relu_padded, int B, int Y, int X, int Cin, int Cout,
                           int relu, void *stream);
/* The same with stride 2 (Conv2d(k = 3, stride = 2, padding = 1): DPTHead.resize_layers[3],
 * depth_anything/dpt.py:69-72): in = padded image (B, Cin, Yin, Xin), out = padded image
 * (B, Cout, ceil(Yin/2), ceil(Xin/2)); only the needed output pixels are computed (the
 * activation rows of a tile are gathered by per-lane DMA addresses). */
int veon_conv2d_k3s2_bf16(const void *in_padded, const void *w_bf16, const float *scale,
                          const float *shift, const void *resid_padded, void *out_padded,
                          int B, int Yin, int Xin, int Cin, int Cout, int act,
                          void *stream);

/* Host-only: the (rows | cols << 16) tile the conv launcher picks for a problem
 * (kd = 3: veon_conv3d_k3_bf16 on B x Z x Y x X voxels; kd = 1: the 2-D convs on
 * B x Y x X output pixels, stride 1 or 2); -1 for an unsupported shape.  Lets the CPU
 * tests pin the selection rule (csrc/conv3d.hip: conv_pick_tile). */
int veon_conv_tile_choice(int kd, int B, int Z, int Y, int X, int Cin, int Cout, int stride);

/* (B,C,Y,X) fp32 or bf16 (nchw_is_bf16) <-> interior of the padded image grid */
int veon_image_pack_bf16(const void *nchw, int nchw_is_bf16, void *padded, int B,
                         int C, int Y, int X, void *stream);
int veon_image_unpack(const void *padded, void *nchw, int nchw_is_bf16, int B,
                      int C, int Y, int X, void *stream);
/* F.interpolate(mode='bilinear', align_corners=True) between two padded images
 * (interior written only; C % 8 == 0). */
int veon_image_resize_bilinear(const void *in_padded, void *out_padded, int B,
                               int C, int Yi, int Xi, int Yo, int Xo,
                               void *stream);

/* ViT token rows -> padded image, with the pixel shuffle of a ConvTranspose2d(k = s,
 * stride = s) folded in (DPTHead.resize_layers[0:2], depth_anything/dpt.py:55-72:
 * the transposed convolution itself is a GEMM over the tokens whose output row holds
 * the s*s pixels [i][j][C] of one token).  rows: bf16 [B*tokens_per_image][row_elems]
 * (row_elems >= s*s*C); the first ``skip`` rows of every image (class token) are
 * passed over; out: padded image (B, C, s*h, s*w), interior written.  C % 8 == 0. */
int veon_tokens_to_image(const void *rows, int64_t row_elems, int tokens_per_image,
                         int skip, int h, int w, int s, int C, void *out_padded, int B,
                         void *stream);
/* out(y,x) = in(step*y, step*x) between padded images (B,C,Yi,Xi) ->
 * (B,C,ceil(Yi/step),ceil(Xi/step)): a stride-``step`` 3x3 pad-1 convolution
 * (DPTHead.resize_layers[3]) is veon_conv2d_k3_bf16 followed by this. */
int veon_image_subsample(const void *in_padded, void *out_padded, int B, int C, int Yi,
                         int Xi, int step, void *stream);
/* out (B,Y,X) fp32 = act(1x1 conv C -> 1 of a padded image + bias); C in {32, 64};
 * act 0 none / 1 ReLU / 2 sigmoid (the tail of DPTHead.output_conv2, dpt.py). */
int veon_image_dot(const void *in_padded, const float *w, float bias, float *out,
                   int B, int C, int Y, int X, int act, void *stream);

/* LayerNorm over the channels of every pixel of a padded channels-last bf16 image:
 * the nn.LayerNorm calls of ConvBlock.forward (highres_side_adaptor.py:31-52) with
 * their permute / reshape pairs.  out_tokens_f32 = 0: out is a padded bf16 image of
 * the same shape, halo written as zeros (input of the next 3x3 conv); 1: out is the
 * compact fp32 token tensor (B, Y*X, C), plus resid_tokens (same shape, fp32, may
 * be NULL): the `ConvBlock(ln_3(x)) + x` of the adaptor block (:122).
 * C % 8 == 0, C <= 1024. */
int veon_image_layernorm_bf16(const void *in_padded, const float *gamma,
                              const float *beta, void *out, int out_tokens_f32, int B,
                              int C, int Y, int X, float eps, const float *resid_tokens,
                              void *stream);

/* (B,C,Z,Y,X) fp32 <-> interior of the padded channels-last bf16 grid (the halo
 * is not touched: allocate the grid zeroed once). */
int veon_volume_pack_bf16(const float *ncdhw, void *padded, int B, int C, int Z,
                          int Y, int X, void *stream);
int veon_volume_unpack_f32(const void *padded, float *ncdhw, int B, int C, int Z,
                           int Y, int X, void *stream);

/* ======== temporal.hip ============================================================== */

/* ---- temporal path, csrc/temporal.hip ---------------------
 * Sampling + attention core of TemporalDeformable.forward
 * (mmdet3d/models/semantic_net/side_adapter/align_net_occ3d.py:138-196), replacing
 * its repeat + F.grid_sample + two einsums + softmax.  All operands are padded
 * channels-last bf16 grids of one (B,Z,Y,X) shape: kv has 2*C channels laid out
 * per head as [key hd | value hd] (the reference's view of key_value_proj), q has
 * C, off has off_channels >= heads*samples*3 raw (pre-tanh) offsets ordered
 * (head, sample, axis); out (C channels) gets its interior rows written, the
 * halo is not touched.  samples must be 8; C/heads in {32, 64}. */
int veon_deform_attention_bf16(const void *kv_padded, const void *q_padded,
                               const void *off_padded, void *out_padded, int B,
                               int Z, int Y, int X, int C, int heads, int samples,
                               int off_channels, void *stream);
/* SANInVeonTemporal.align_after_lss (san_in_veon_temporal.py:325-365) on a padded
 * grid: out voxel (x,y,z) = trilinear sample of `in` at affine[b] (3x4 row-major,
 * voxel-index units) applied to (x,y,z,1); zero outside (F.grid_sample
 * padding_mode='zeros', align_corners=True). */
int veon_volume_warp_bf16(const void *in_padded, void *out_padded,
                          const float *affine, int B, int C, int Z, int Y, int X,
                          void *stream);
/* The coordinate chain of align_after_lss (san_in_veon_temporal.py:326-358) as one
 * 3x4 map in voxel-index units per sample, computed on the device in double:
 * affine[b] = S^-1 inv(prev2glob[b]) cur2glob[b] S, S = diag(step) + first voxel
 * centre.  cur2glob / prev2glob: device fp32 4x4 row-major, mat_stride floats
 * apart (>= 16); first_xyz / step_xyz: HOST doubles[3]; affine: device (B,3,4). */
int veon_warp_affine(const float *cur2glob, const float *prev2glob, int mat_stride,
                     const double *first_xyz, const double *step_xyz, float *affine,
                     int B, void *stream);
/* zero the halo rows of a padded grid (after a row-wise GEMM epilogue wrote its
 * shift there and a 3x3x3 conv is to consume it). */
int veon_volume_zero_halo_bf16(void *padded, int B, int C, int Z, int Y, int X,
                               void *stream);

/* ======== conv3d_train.hip ========================================================== */

/*
 * ---- training of the Conv3d body on the padded grid (ResBlock3D with BN3d in training
 * mode, align_net_occ3d.py:224-264, 363-399) ----
 * All volumes are padded channels-last half grids as veon_conv3d_k3_bf16 takes and
 * writes them, with the same guard rows, which must hold ZEROS here (they enter the
 * weight gradient's contraction; a PaddedVolume allocates them zeroed and no kernel
 * writes them).  The data gradient needs no entry point of its own: it is
 * veon_conv3d_k3_bf16 on dy with the weight packed as [Cin][2-kz][2-ky][2-kx][Cout].
 *
 * Weight gradient: dw[co][kz][ky][kx][ci] (fp32) = sum over ALL padded rows of
 * dy[row][co] * x[row + off(kz,ky,kx)][ci]; halo rows of dy are zero, so this is the
 * sum over the interior.  MFMA with transposed LDS reads of both operands; the
 * contraction is split over the rows, the partial results go to fp32 slabs in
 * `workspace` (veon_conv3d_k3_wgrad_workspace_bytes, host-only; -1 for an unsupported
 * shape) and are added in a fixed order: no atomics, bit-reproducible.
 * Cin % 64 == 0 and Cout % 64 == 0, otherwise VEON_ERR_BAD_ARG; a workspace that is
 * too small gives VEON_ERR_WORKSPACE.
 */
int64_t veon_conv3d_k3_wgrad_workspace_bytes(int B, int Z, int Y, int X, int Cin, int Cout);
int veon_conv3d_k3_wgrad_bf16(const void *dy_padded, const void *x_padded, float *dw,
                              void *workspace, int64_t workspace_bytes, int B, int Z,
                              int Y, int X, int Cin, int Cout, void *stream);

/*
 * Train-mode BatchNorm3d on padded rows.  Per-channel sums over all padded rows in
 * fp32, two stages, fixed order (halo rows are zero, so they are the interior's sums):
 *   veon_bn3d_sums_bf16:     sums[0][c] = sum y,  sums[1][c] = sum y^2
 *   veon_bn3d_bwd_sums_bf16: sums[0][c] = sum dz, sums[1][c] = sum dz * xhat, with
 *                            dz = da * [a > 0], xhat = (y - mean[c]) * rstd[c]
 * `workspace`: veon_bn3d_sums_workspace_bytes(C) bytes (host-only; -1: unsupported C).
 *   veon_bn3d_apply_bf16:     out = y * scale[c] + shift[c] (+ ident) (ReLU if `relu`)
 *   veon_bn3d_bwd_apply_bf16: dz as above, dy = ca[c] * dz + cb[c] * y + cc[c];
 *                             dz_padded (optional) receives dz, the gradient of the
 *                             identity branch
 * on interior rows, ZERO on halo rows, rounded to half.  C % 8 == 0, C <= 2048.
 * Outputs must not alias inputs.
 */
int64_t veon_bn3d_sums_workspace_bytes(int C);
int veon_bn3d_sums_bf16(const void *y_padded, float *sums, void *workspace, int B, int C,
                        int Z, int Y, int X, void *stream);
int veon_bn3d_bwd_sums_bf16(const void *da_padded, const void *a_padded,
                            const void *y_padded, const float *mean, const float *rstd,
                            float *sums, void *workspace, int B, int C, int Z, int Y,
                            int X, void *stream);
int veon_bn3d_apply_bf16(const void *y_padded, const float *scale, const float *shift,
                         const void *ident_padded, void *out_padded, int relu, int B,
                         int C, int Z, int Y, int X, void *stream);
int veon_bn3d_bwd_apply_bf16(const void *da_padded, const void *a_padded,
                             const void *y_padded, const float *ca, const float *cb,
                             const float *cc, void *dy_padded, void *dz_padded, int B,
                             int C, int Z, int Y, int X, void *stream);

/*
 * Synchronised train-mode BatchNorm3d (nn.SyncBatchNorm): the statistics interval as a
 * message.  Stage one of the sums is that of veon_bn3d_sums_bf16 / veon_bn3d_bwd_sums_bf16
 * (same plan, same workspace); stage two adds the fp32 partials in fp64, many workgroups,
 * a fixed assignment of partials to lanes and a fixed-order combine: no atomics, no memset,
 * bit-reproducible whatever `workspace` and `stats` held.
 *   stats[2C + 1] (fp64): the two sums of the plain entry point, then the LOCAL count
 *   n = B Z Y X.  Ranks add their buffers elementwise (one all-reduce); the coefficient
 *   calls below read the total count from the buffer on the device.
 *   veon_bn3d_bwd_sums_stats_bf16 also writes the local sums rounded to fp32 to
 *   sums[2][C] (dbeta, dgamma: they stay per rank).
 * veon_bn_train_coeffs, one launch: mean = s0 / n, var = max(s1 / n - mean^2, 0),
 * rstd = (var + eps)^-1/2, scale = gamma rstd, shift = beta - mean scale (fp64, stored
 * fp32).  With running buffers (all three or none): num_batches_tracked += 1, then
 * running = (1 - f) running + f value with f = momentum, or 1 / num_batches_tracked when
 * momentum < 0 (nn.BatchNorm's momentum=None); the values are mean (+ mean_offset[c] when
 * given: a conv bias that was not added to y) and var n / (n - 1).
 * veon_bn_bwd_coeffs, one launch: ca = gamma rstd, cb = -gamma rstd^2 s1 / n,
 * cc = -gamma rstd s0 / n - cb mean, the vectors of veon_bn3d_bwd_apply_bf16.
 * C % 8 == 0, C <= 2048; stats 8-byte aligned.
 */
int veon_bn3d_sums_stats_bf16(const void *y_padded, double *stats, void *workspace, int B,
                              int C, int Z, int Y, int X, void *stream);
int veon_bn3d_bwd_sums_stats_bf16(const void *da_padded, const void *a_padded,
                                  const void *y_padded, const float *mean,
                                  const float *rstd, double *stats, float *sums,
                                  void *workspace, int B, int C, int Z, int Y, int X,
                                  void *stream);
int veon_bn_train_coeffs(const double *stats, const float *gamma, const float *beta,
                         const float *mean_offset, double eps, double momentum,
                         float *running_mean, float *running_var,
                         int64_t *num_batches_tracked, float *mean, float *rstd,
                         float *scale, float *shift, int C, void *stream);
int veon_bn_bwd_coeffs(const double *stats, const float *gamma, const float *mean,
                       const float *rstd, float *ca, float *cb, float *cc, int C,
                       void *stream);

/* ======== conv2d_train.hip ========================================================== */

/*
 * ---- training of the HSA ConvBlock on padded images (conv3x3 + bias -> GELU -> LN ->
 * conv3x3 + bias -> LN, highres_side_adaptor.py:31-52) ----
 * All images are padded channels-last half grids [B][Y+2][X+2][C] as veon_conv2d_k3_bf16
 * takes and writes them, with veon_conv3d_guard_rows(Y, X) guard rows before and after.
 * The GUARD ROWS OF x MUST HOLD ZEROS for the weight gradient (they enter its
 * contraction; a PaddedImage allocates them zeroed and no kernel writes them).  The data
 * gradient needs no entry point of its own: it is veon_conv2d_k3_bf16 on dy with the
 * weight packed as [Cin][2-ky][2-kx][Cout].
 *
 * Weight gradient: dw[co][ky][kx][ci] (fp32) = sum over ALL padded rows of
 * dy[row][co] * x[row + (ky-1)(X+2) + (kx-1)][ci]; halo rows of dy are zero, so this is
 * the sum over the interior.  The kernel of veon_conv3d_k3_wgrad_bf16 with one ky per
 * workgroup; split over the rows into fp32 slabs of `workspace`
 * (veon_conv2d_k3_wgrad_workspace_bytes, host-only; -1 for an unsupported shape), added
 * in index order: no atomics, bit-reproducible.  Cin % 64 == 0 and Cout % 64 == 0,
 * otherwise VEON_ERR_BAD_ARG; a workspace that is too small gives VEON_ERR_WORKSPACE.
 */
int64_t veon_conv2d_k3_wgrad_workspace_bytes(int B, int Y, int X, int Cin, int Cout);
int veon_conv2d_k3_wgrad_bf16(const void *dy_padded, const void *x_padded, float *dw,
                              void *workspace, int64_t workspace_bytes, int B, int Y,
                              int X, int Cin, int Cout, void *stream);

/*
 * out = LayerNorm(GELU(in)) over the channels of every pixel: GELU in its erf form in
 * fp32 from the stored half value, statistics in fp32, halo rows written as ZEROS (the
 * next conv's padded input).  C % 8 == 0, C <= 1024, as veon_image_layernorm_bf16.
 */
int veon_image_gelu_layernorm_bf16(const void *in_padded, const float *gamma,
                                   const float *beta, void *out_padded, int B, int C,
                                   int Y, int X, float eps, void *stream);

/*
 * Backward of that LayerNorm in one pass over the rows; the row statistics are
 * recomputed from the LayerNorm's stored input x_padded (`gelu_in` != 0: the
 * LayerNorm's input was GELU(x), and dx is the gradient of x, through GELU' too).
 * `dout`: a padded half image (dout_tokens_f32 == 0) or compact fp32 tokens
 * (B, Y*X, C).  dx_padded: padded half image, halo rows written as ZEROS.
 * sums[3][C] (fp32) over the interior rows: [0] dgamma = sum dout * xhat,
 * [1] dbeta = sum dout, [2] sum dx (the gradient of the bias of the conv in front; fp32
 * values, before dx is rounded to half).  Two stages in a fixed order, no atomics;
 * `workspace`: veon_image_layernorm_bwd_workspace_bytes(C) bytes (host-only; -1:
 * unsupported C).  C % 8 == 0, C <= 1024.  Outputs must not alias inputs.
 */
int64_t veon_image_layernorm_bwd_workspace_bytes(int C);
int veon_image_layernorm_bwd_bf16(const void *dout, int dout_tokens_f32,
                                  const void *x_padded, int gelu_in, const float *gamma,
                                  void *dx_padded, float *sums, void *workspace,
                                  int64_t workspace_bytes, int B, int C, int Y, int X,
                                  float eps, void *stream);

/* ======== linear_train.hip ========================================================== */

/*
 * ---- training of the HSA FeedForward heads (LN -> Linear -> GELU -> Linear,
 * highres_side_adaptor.py:55-66) and of the blocks' token LayerNorms on plain rows ----
 * Rows are ordinary contiguous matrices WITHOUT guard rows; M (T) is any positive count.
 *
 * Weight gradient of a linear layer y = x W^T: dw[n][k] (fp32, the nn.Linear layout) =
 * sum over the M rows of dy[row][n] * x[row][k], dy half [M][N], x half [M][K].  The
 * kernel of veon_conv3d_k3_wgrad_bf16 as its one-tap case: one workgroup per tile and
 * split of the rows, fp32 slabs of `workspace` (veon_linear_wgrad_workspace_bytes,
 * host-only; -1 for an unsupported shape) added in index order: no atomics,
 * bit-reproducible.  Rows >= M are never read (bounded buffer resources) and contribute
 * exactly zero.  K % 64 == 0, N % 64 == 0 and M * max(K, N) < 2^30, otherwise
 * VEON_ERR_BAD_ARG; a workspace that is too small gives VEON_ERR_WORKSPACE.
 */
int64_t veon_linear_wgrad_workspace_bytes(int M, int K, int N);
int veon_linear_wgrad_bf16(const void *dy, const void *x, float *dw, void *workspace,
                           int64_t workspace_bytes, int M, int K, int N, void *stream);

/*
 * The bias gradient: sums[N] (fp32) = sum over the M rows of dy half [M][N].  Two stages
 * in a fixed order, no atomics; `workspace`: veon_rows_colsum_workspace_bytes(N) bytes
 * (host-only; -1: unsupported N).  N % 8 == 0.
 */
int64_t veon_rows_colsum_workspace_bytes(int N);
int veon_rows_colsum_bf16(const void *dy, float *sums, void *workspace,
                          int64_t workspace_bytes, int M, int N, void *stream);

/*
 * h = GELU(y) and dy = dh * GELU'(y), GELU'(y) = Phi(y) + y phi(y), elementwise on n half
 * values (n % 8 == 0): the erf form in fp32 from the stored half value, both from one
 * erfc evaluation, as veon_image_layernorm_bwd_bf16's gelu_in.  Outputs must not alias
 * inputs.
 */
int veon_gelu_bf16(const void *y, void *h, int64_t n, void *stream);
int veon_gelu_bwd_bf16(const void *dh, const void *y, void *dy, int64_t n, void *stream);

/*
 * The same pair for CLIP's QuickGELU: h = y * sigma(1.702 y) and
 * dy = dh * (sigma + 1.702 * y * sigma * (1 - sigma)), sigma = sigmoid(1.702 y), in fp32
 * from the stored half pre-activation.  n % 8 == 0; outputs must not alias inputs.
 */
int veon_quickgelu_bf16(const void *y, void *h, int64_t n, void *stream);
int veon_quickgelu_bwd_bf16(const void *dh, const void *y, void *dy, int64_t n,
                            void *stream);

/*
 * Backward of nn.LayerNorm over the last axis at its stored fp32 input x [T][d]; the row
 * statistics are recomputed.  `dout`: fp32 [T][d] (dout_half == 0) or half [T][d].
 * dx fp32 [T][d]; sums[2][d] (fp32): [0] dgamma = sum dout * xhat, [1] dbeta = sum dout.
 * Two stages in a fixed order, no atomics; `workspace`:
 * veon_layernorm_f32_bwd_workspace_bytes(d) bytes (host-only; -1: unsupported d).
 * d % 64 == 0, d <= 1024.  dx must not alias an input.
 */
int64_t veon_layernorm_f32_bwd_workspace_bytes(int d);
int veon_layernorm_f32_bwd(const void *dout, int dout_half, const float *x,
                           const float *gamma, float *dx, float *sums, void *workspace,
                           int64_t workspace_bytes, int T, int d, float eps, void *stream);

/* ======== attention_train.hip ======================================================= */

/*
 * Attention for training, head_dim 64, no additive bias.  qkv half [B][T][3][H][64] is
 * the RAW output of the qkv Linear: the kernels multiply the scores by `scale`, so every
 * gradient comes out in the parameters' own units.
 *
 * veon_vit_attention_fwd_lse: out half [B][T][H*64] = softmax(scale q k^T) v by the
 * inference kernel, and lse[b][h][q] (fp32) = log2 sum_k exp2(scale log2(e) q.k), the
 * log-sum-exp of the scaled scores in log2 units.  Rows of lse are
 * veon_vit_attention_stats_len(T) floats (T rounded up to 64; 0: T <= 0), so lse holds
 * B * H * stats_len floats; columns T.. of a row are not written.
 *
 * veon_vit_attention_bwd: dqkv half [B][T][3][H][64] from dout half [B][T][H*64] and the
 * saved qkv, out and lse.  Three kernels: delta = rowsum(dout * out) into the workspace
 * (veon_vit_attention_bwd_workspace_bytes(B, T, H) bytes, host-only; -1: bad shape), dq,
 * and dk with dv.  Every element of dqkv is written; no atomics, no memset; columns T..
 * of lse and of the workspace rows are never used.  dqkv must not alias an input.
 */
int64_t veon_vit_attention_stats_len(int T);
int veon_vit_attention_fwd_lse(const void *qkv, void *out, float *lse, int B, int T, int H,
                               int head_dim, float scale, void *stream);
int64_t veon_vit_attention_bwd_workspace_bytes(int B, int T, int H);
int veon_vit_attention_bwd(const void *qkv, const void *out, const void *dout,
                           const float *lse, void *dqkv, void *workspace,
                           int64_t workspace_bytes, int B, int T, int H, int head_dim,
                           float scale, void *stream);

/*
 * The same pair with a dense additive bias (the CLIP tail under autograd).  qkv, out, lse,
 * scale and the workspace are exactly those of the unbiased pair: raw q, lse in log2 units
 * in rows of veon_vit_attention_stats_len(T) floats, columns T.. never used.
 *
 * `bias`: fp32, natural-log units, added to scale * q.k.  Per (b, h) it is a [Tb][Tb]
 * matrix, Tb = T - border, rows Tb floats long (no alignment requirement on Tb), at
 * bias + b * bias_sb + h * bias_sh (element strides >= 0; 0 broadcasts the axis).
 * `border` is 0 or 1.  With border = 1 the matrix is patch-to-patch: token 0 (the class
 * token) has bias 0 as a query and as a key, by index, and nothing outside [0, Tb)^2 of a
 * matrix is read or written.  T = 1 with border = 1 is legal: the bias is never read and
 * may be NULL.
 *
 * veon_vit_attention_bias_fwd_lse: out = softmax(scale q k^T + bias) v and
 * lse[b][h][q] = log2 sum_k exp2((scale q.k + bias) log2(e)).
 *
 * veon_vit_attention_bias_bwd: dqkv as veon_vit_attention_bwd gives it, and
 * dbias[B][H][Tb][Tb] (fp32, always dense, also for a broadcast bias: the caller sums)
 * = dS = P o (dP - delta), the gradient with respect to the bias (no `scale` factor).
 * Every element of both is written exactly once; no atomics, no memset.  dbias == NULL
 * skips its stores.  The delta pass of this pair is delta[q] = sum_k P dP / sum_k P from
 * the rebuilt probabilities themselves (one more sweep over the keys), not
 * rowsum(dout * out): on the saturated rows a bias with a large diagonal makes, the half
 * rounding of `out` would be several times the row's whole dS.  `out` is part of the
 * interface (it is what the forward saved, as in the unbiased pair) and must be valid, but
 * is not read.  dqkv == NULL (nothing upstream of the qkv Linear needs a gradient) runs
 * only the delta pass and the dS pass: no dq accumulation, no dk / dv launch.  Both NULL
 * is VEON_ERR_BAD_ARG.  dqkv and dbias must not alias an input.
 *
 * Masks: a bias of -inf gives the key p = 0, ds = 0, dbias = 0.  A query whose keys are
 * ALL masked has an out row of zeros (as the inference kernel gives) and lse = +inf, so
 * that the backward's exp2(... - lse) is exactly 0 for it: its dq row and its dbias row are
 * zero, it adds nothing to any dk or dv, and nothing is NaN.
 */
int veon_vit_attention_bias_fwd_lse(const void *qkv, const float *bias, int64_t bias_sb,
                                    int64_t bias_sh, int border, void *out, float *lse,
                                    int B, int T, int H, int head_dim, float scale,
                                    void *stream);
int veon_vit_attention_bias_bwd(const void *qkv, const float *bias, int64_t bias_sb,
                                int64_t bias_sh, int border, const void *out,
                                const void *dout, const float *lse, void *dqkv,
                                float *dbias, void *workspace, int64_t workspace_bytes,
                                int B, int T, int H, int head_dim, float scale,
                                void *stream);

/* ======== temporal_train.hip ======================================================== */

/*
 * Backward of veon_deform_attention_bf16, the sampling + attention core of
 * TemporalDeformable.forward (align_net_occ3d.py:138-196), with the same operands, shape
 * limits and meaning of `off_padded` (RAW offsets, off_channels >= heads*samples*3, the
 * surplus ignored).  The forward stores nothing: positions are recomputed bit for bit.
 * `workspace`: veon_deform_attention_bwd_workspace_bytes(B, Z, Y, X, heads) bytes
 * (host-only; -1: bad shape), 64 bytes per (voxel, head): the fp32 pairs
 * (hd^-0.5 dlogit_s, softmax weight_s) of the 8 samples.
 *
 * veon_deform_attention_bwd_bf16 (align_net_occ3d.py:138-196): from dout (C channels)
 * writes dq (C channels) and doff (off_channels channels: the gradient of the RAW offsets,
 * through tanh; surplus channels zero) with ZERO halos, and the workspace.  ATen's
 * grid_sample conventions: no offset gradient on an axis whose clamped coordinate lies on
 * or beyond the border (f <= 0 or f >= n - 1), the right-hand derivative at a node.
 *
 * veon_deform_attention_bwd_dkv_bf16 (align_net_occ3d.py:138-196): dkv (2*C channels, every
 * row written, halo zero) from the workspace the call above filled.  `ranges`: DEVICE ints,
 * (lo, hi) inclusive pairs (hi < lo: empty), X pairs of source z indices per target x, then
 * Y pairs of source y per target y, then Z pairs of source x per target z: a superset of
 * the voxels whose samples can touch that target coordinate (the X position of a sample is
 * driven by its voxel's z index, the Z position by x).  A gather over that box in a fixed
 * order: no atomics, repeated calls are bit-identical.  Outputs must not alias inputs.
 */
int64_t veon_deform_attention_bwd_workspace_bytes(int B, int Z, int Y, int X, int heads);
int veon_deform_attention_bwd_bf16(const void *kv_padded, const void *q_padded,
                                   const void *off_padded, const void *dout_padded,
                                   void *dq_padded, void *doff_padded, void *workspace,
                                   int64_t workspace_bytes, int B, int Z, int Y, int X,
                                   int C, int heads, int samples, int off_channels,
                                   void *stream);
int veon_deform_attention_bwd_dkv_bf16(const void *q_padded, const void *off_padded,
                                       const void *dout_padded, const void *workspace,
                                       int64_t workspace_bytes, const int *ranges,
                                       void *dkv_padded, int B, int Z, int Y, int X, int C,
                                       int heads, int samples, int off_channels,
                                       void *stream);

/* ======== occ_tail.hip ============================================================== */

/* Tail of the occupancy path in one kernel (semantic_net/san_in_veon_temporal.py:
 * 196-211 + detectors/veon_temporal.py:219-227): sem (B,Q,zi,yi,xi) and bin
 * (B,2,zi,yi,xi) fp32 logits, each addressed through five ELEMENT strides
 * {b, c, z, y, x} (so the channels-last rows of the heads' GEMMs are read in place),
 * are upsampled trilinearly (align_corners=False) to (Zo,Yo,Xo):
 *   sem_out (B,Q,Zo,Yo,Xo), bin_out (B,2,Zo,Yo,Xo) fp32 contiguous,
 *   cls_out (B,Xo,Yo,Zo) int64 = argmax_c softmax(sem_out) where
 *     softmax(bin_out)[0] > 0.5 (and the best score > 0), else Q (= free). */
int veon_occ_classify(const float *sem, const int64_t *sem_strides, int Q,
                      const float *bin, const int64_t *bin_strides, int B, int zi,
                      int yi, int xi, int Zo, int Yo, int Xo, float *sem_out,
                      float *bin_out, int64_t *cls_out, void *stream);

/* ======== occ_tail.hip (veon_occ_labels), occ_eval.hip (veon_occ_confusion) ========= */

/* The label-only tail: what VEONTemporal.simple_test returns (detectors/
 * veon_temporal.py:219-241 keeps only occ_pred_cls, as uint8).  Inputs, strides, extent
 * checks and the label rule are those of veon_occ_classify (first maximum of the class
 * logits where they hold no NaN and a finite maximum and softmax(bin)[0] > 0.5, else
 * Q), computed by the same code: labels (B,Xo,Yo,Zo) uint8 are bit-equal to its cls_out
 * and are the ONLY output.  1 <= Q <= 254, Zo <= 2048.
 * Optionally the confusion matrix of Metric_mIoU (mmdet3d/datasets/occ_metrics.py:
 * 78-147, hist_info after add_batch's masking) in the same pass: gt (B,Xo,Yo,Zo) uint8
 * and hist (n_cl*n_cl int64, n_cl = Q + 1 <= 64) are given together or both NULL; mask
 * (B,Xo,Yo,Zo) uint8, 0 = skip, NULL = no mask.  Every voxel with mask != 0 and
 * gt < n_cl adds 1 to hist[n_cl*gt + label] (gt = 255, "ignore", falls out by the range
 * test).  hist is ACCUMULATED into, never cleared: the metric's state stays on the device
 * across samples.  Integer atomics: exact, the same for every run.  Nothing is allocated
 * or read back. */
int veon_occ_labels(const float *sem, const int64_t *sem_strides, int Q, const float *bin,
                    const int64_t *bin_strides, int B, int zi, int yi, int xi, int Zo,
                    int Yo, int Xo, uint8_t *labels, const uint8_t *gt,
                    const uint8_t *mask, int64_t *hist, void *stream);

/* The same confusion matrix for labels that exist already (occ_metrics.py:78-147): pred
 * holds n labels of pred_elem_bytes = 1 (uint8) or 8 (int64, veon_occ_classify's
 * cls_out) in the order of gt (n uint8) and mask (n uint8, 0 = skip, NULL = no mask);
 * 1 <= n < 2^31, 1 <= n_cl <= 64.  Every voxel with mask != 0 and gt < n_cl adds 1 to
 * hist[n_cl*gt + pred] (n_cl*n_cl int64, accumulated into); such a voxel whose
 * prediction is outside [0, n_cl) counts in no bin and sets *flag (a device int, may be
 * NULL; never cleared here) to 1. */
int veon_occ_confusion(const void *pred, int pred_elem_bytes, const uint8_t *gt,
                       const uint8_t *mask, int64_t n, int n_cl, int64_t *hist, int *flag,
                       void *stream);

/* ======== occ_tail.hip: the grouped tails =========================================== */

/* The two tails against a detailed vocabulary (SANInVeonTemporal._merge_classes_prob,
 * san_in_veon_entry_temporal.py:273-297, then veon_temporal.py:220-229): sem holds K
 * low-resolution logit rows (strides, extents and interpolation as veon_occ_classify),
 * group (a HOST array of K bytes) names the merged channel of each row.
 *   - The rows of one merged channel are CONSECUTIVE, and every channel in [0, n_merged)
 *     has exactly one run; which run feeds which channel is otherwise free (the
 *     background run may come first or last).  Anything else: VEON_ERR_BAD_ARG.
 *   - merged value = the maximum over the run's UPSAMPLED rows, NaN if one of them is NaN
 *     (torch.max);
 *   - label = the lowest merged channel that attains the maximum merged value;
 *   - scored = no NaN in any of the K rows and a finite maximum;
 *     keep = scored and softmax(upsampled bin)[0] > 0.5; a voxel that is not kept gets
 *     free_label (0 <= free_label <= 255, need not be n_merged - 1).
 *   - 1 <= K <= 256, 1 <= n_merged <= 64, B*Zo*Yo*Xo < 2^31.
 * The K upsampled rows are never written.  No memset, no allocation, no read-back; every
 * output element is written; the only atomics are the histogram's integer ones.
 *
 * veon_occ_labels_grouped: labels (B,Xo,Yo,Zo) uint8 only, Zo <= 2048; gt / mask / hist as
 * veon_occ_labels with n_cl = max(n_merged, free_label + 1) <= 64: hist (n_cl*n_cl int64)
 * is accumulated into. */
int veon_occ_labels_grouped(const float *sem, const int64_t *sem_strides, int K,
                            const uint8_t *group, int n_merged, int free_label,
                            const float *bin, const int64_t *bin_strides, int B, int zi,
                            int yi, int xi, int Zo, int Yo, int Xo, uint8_t *labels,
                            const uint8_t *gt, const uint8_t *mask, int64_t *hist,
                            void *stream);

/* veon_occ_classify_grouped: the same labels as cls_out (B,Xo,Yo,Zo) int64, the upsampled
 * occupancy pair bin_out (B,2,Zo,Yo,Xo) and the MERGED logits merged_out
 * (B,n_merged,Zo,Yo,Xo) fp32, each channel stored once, when its run ends. */
int veon_occ_classify_grouped(const float *sem, const int64_t *sem_strides, int K,
                              const uint8_t *group, int n_merged, int free_label,
                              const float *bin, const int64_t *bin_strides, int B, int zi,
                              int yi, int xi, int Zo, int Yo, int Xo, float *merged_out,
                              float *bin_out, int64_t *cls_out, void *stream);

/* ======== occ_fscore.hip ============================================================ */

/* The counts of Metric_FScore (mmdet3d/datasets/occ_metrics.py:150-237) without its
 * KD-trees: both point sets are voxel centres of one lattice, so "nearest neighbour
 * closer than the threshold" is an integer stencil (veon_amd/occ_eval.py: fscore_reach).
 * pred: labels (B,X,Y,Z) of pred_elem_bytes = 1 (uint8) or 8 (int64); gt, mask (NULL = no
 * mask): uint8 of the same shape; 1 <= Z <= 64, B*X*Y*Z < 2^31.  A voxel is OCCUPIED
 * when its mask is not 0 and its label is not void; void_words: a HOST array of four
 * 64-bit words, bit v % 64 of word v / 64 set = label v is void; an int64 label outside
 * [0, 255] is occupied.  reach_acc / reach_cmpl: HOST arrays of (2r + 1)^2 ints, r =
 * r_acc / r_cmpl in [0, 3]: entry (dx + r)*(2r + 1) + dy + r is the largest |dz| at which
 * offset (dx, dy, dz) counts as near, in [0, 63], or -1 for none.  Added to
 * counts[4*b ..] (B*4 int64, accumulated into, never cleared):
 *   n_pred, n_gt   occupied voxels of pred / gt in sample b
 *   hit_pred       occupied pred voxels with an occupied gt voxel near (reach_acc)
 *   hit_gt         occupied gt voxels with an occupied pred voxel near (reach_cmpl)
 * Voxels outside the sample's grid are empty.  Nothing is written to the inputs (the
 * reference overwrites masked voxels of its arguments with 255).  Integer atomics:
 * exact, the same for every run.  Nothing is allocated or read back. */
int veon_occ_fscore_counts(const void *pred, int pred_elem_bytes, const uint8_t *gt,
                           const uint8_t *mask, int B, int X, int Y, int Z,
                           const int64_t *void_words, int r_acc, const int *reach_acc,
                           int r_cmpl, const int *reach_cmpl, int64_t *counts,
                           void *stream);

/* ======== occ_retrieval.hip ========================================================= */

/* Open-vocabulary point retrieval, the `retrieval=True` branch of
 * VEONTemporal.simple_test (detectors/veon_temporal.py:232-241, 331-356;
 * semantic_net/san_in_veon_temporal.py:195-200, 212, 268-273), without forming the
 * upsampled feature volume.  feat (B,C,zi,yi,xi): feat_is_half = 1 -> the half type
 * of the build (e.g. the channels-last interior of a padded volume), 0 -> fp32; both
 * addressed through five ELEMENT strides {b, c, z, y, x} (>= 0).  bin (B,2,zi,yi,xi)
 * fp32, any strides.  points: P int32 triples (x, y, z) in the grid (Zo,Yo,Xo), all
 * of batch element `batch` (datasets/pipelines/loading.py:990-1012).  emb (Q,C) fp32
 * contiguous prompt embeddings; emb_norms: a workspace of Q floats.  For every point
 * p and prompt q, with f = trilinear (align_corners=False) upsample of feat at p:
 *   score[q*P + p] = f.e_q / (max(|f|, 1e-8) * max(|e_q|, 1e-8))
 *   bin_prob[p]    = softmax(upsampled bin at p)[0]     (bin_prob NULL: skipped)
 * Points outside the grid get NaN; nothing is read for them.  1 <= C <= 1024, Q >= 1;
 * channels-last rows must hold C channels (C <= x stride).  No atomics: repeated calls
 * are bit-identical. */
int veon_occ_retrieve(const void *feat, int feat_is_half, const int64_t *feat_strides,
                      int C, const float *bin, const int64_t *bin_strides, int B, int zi,
                      int yi, int xi, int Zo, int Yo, int Xo, const int *points, int P,
                      int batch, const float *emb, int Q, float *emb_norms, float *score,
                      float *bin_prob, void *stream);

/* ======== occ_align_loss.hip ======================================================== */

/* The differentiable primitive of the 2D->3D feature-alignment loss (Proj2Dto3DLoss,
 * models/semantic_net/loss/occ_loss_utils/occ3d_nuscenes.py:454-461, 497-504) from the
 * LOW-resolution feature volume: the upsampled volume (san_in_veon_temporal.py:196-200)
 * is formed in neither direction.  feat (B,C,zi,yi,xi) fp32 through five ELEMENT strides
 * {b, c, z, y, x}; voxels: N int32 triples (x, y, z) in the grid (Zo,Yo,Xo), all of batch
 * element `batch`, in any order, repeats allowed; labels: N int32 rows of table (K,C)
 * fp32 contiguous; table_norms: K floats, written.  With f_i = trilinear
 * (align_corners=False) upsample of feat at voxel i and t_i = table[labels_i]:
 *   cos_out[i]     = f_i.t_i / (max(|f_i|, eps) * max(|t_i|, eps))
 *   stats[2i]      = f_i.t_i / max(|t_i|, eps)        stats[2i+1] = |f_i|
 * An entry whose voxel lies outside the grid or whose label lies outside [0, K) reads
 * nothing and gets zeros (the caller refuses such entries beforehand).
 * 1 <= C <= 1024, eps > 0.  No atomics: repeated calls are bit-identical. */
int veon_occ_align_fwd(const float *feat, const int64_t *feat_strides, int C, int B, int zi,
                       int yi, int xi, int Zo, int Yo, int Xo, const int *voxels,
                       const int *labels, int N, int batch, const float *table, int K,
                       float eps, float *table_norms, float *cos_out, float *stats,
                       void *stream);
/* Gradient of sum_i g[i] * cos_out[i] with respect to feat[batch], for the grid
 * (2 zi, 2 yi, 2 xi) only, as autograd returns it for ATen's cosine_similarity:
 *   d cos_i / d f_i = u_i / n_i - (f_i.u_i / n_i^2) * f_i / |f_i|,
 *   n_i = max(|f_i|, eps), u_i = t_i / max(|t_i|, eps), the last factor 0 at f_i = 0.
 * table_norms and stats as the forward wrote them.  The entries arrive grouped by
 * output voxel: order (N) lists the entry indices voxel by voxel, seg_start (M + 1) the
 * bounds of the M distinct voxels' runs in it, occ_rows (2zi * 2yi * 2xi, index
 * (z * Yo + y) * Xo + x) the run of every output voxel or -1.  rows: workspace of M * C
 * floats (one gradient row per distinct voxel).  grad: (zi, yi, xi, C) contiguous, every
 * element stored exactly once (zeros where nothing arrives; no memset needed).  No
 * atomics: the sums run in the order of `order` and of a fixed 64-candidate stencil, so
 * repeated calls are bit-identical. */
int veon_occ_align_bwd(const float *feat, const int64_t *feat_strides, int C, int B, int zi,
                       int yi, int xi, const int *voxels, const int *labels, int N,
                       int batch, const float *table, int K, float eps,
                       const float *table_norms, const float *stats, const float *g,
                       const int *order, const int *seg_start, int M, const int *occ_rows,
                       float *rows, float *grad, void *stream);

/* ======== occ_align_select.hip ====================================================== */

/* The discrete half of the 2D->3D feature-alignment loss (Proj2Dto3DLoss,
 * models/semantic_net/loss/occ_loss_utils/occ3d_nuscenes.py:372-508) for ONE sample: which
 * (camera, voxel) pairs the loss trains on, with which label and weight.  Pairs are
 * numbered camera-major, p = cam * Xo*Yo*Zo + vox, vox = (x * Yo + y) * Zo + z, the linear
 * order of the label tensor; n_cam <= 32, n_cam * Xo*Yo*Zo <= 2^31 - 257, n_cls <= 32.
 * No float atomics and no atomic tickets: every order comes from a scan, repeated calls are
 * bit-identical.  Nothing is read back; the caller reads head[0] after _mark (it sizes the
 * entry arrays) and `result` after _emit.
 *
 * labels: (Xo,Yo,Zo) uint8, or int64 when labels_are_int64 (values outside [0, 255] count
 * as "not a class"); a pair is a candidate when 0 <= label < n_cls.  cams: n_cam * 24
 * floats = rows 0-2 of ego2img (3 x 4, row-major), post_rots (3 x 3), post_trans (3).
 * grid: 10 HOST floats = step and offset (lower bound + step / 2) of x, y, z, then image
 * width - 1, height - 1, depth lower and upper bound.  For a candidate, in fp32,
 *   centre = index * step + offset;  p = ego2img centre;  (a, b) = (p.x, p.y) / p.z;
 *   (u, v, d) = post_rots (a, b, p.z) + post_trans;
 *   kept = 0 <= u <= width - 1 && 0 <= v <= height - 1 && depth_lo <= d < depth_hi.
 *
 * veon_align_select_groups: the number G of 256-pair workgroups (-1: unsupported size).
 * veon_align_select_mark writes masks (4 G 64-bit words: the kept bit of every pair),
 * offsets (G ints: kept pairs in front of each workgroup), head[0] = kept pairs, and clears
 * head[1 .. n_head); n_head >= 4 + 2 n_cam n_cls + n_cam.
 *
 * veon_align_select_classify (n_kept = head[0] >= 1, masks / offsets / head as _mark left
 * them) fills, for kept entry i in pair order: pair[i], voxels[3i..] = (x, y, z),
 * classes[4i..] = {label, plain, merged, restricted}, flags[i] (bit 0 det, bit 1 soft).
 * sem (n_cam,K2,hs,ws) fp32 contiguous is sampled as F.grid_sample(bilinear,
 * align_corners=False, zeros) does at (u / half_w - 1, v / half_h - 1), half_w =
 * (width - 1) / 2: ix = ((x + 1) ws - 1) / 2, corners outside the map contribute 0.
 * gid (K2 ints): merged class of every 2-D class, non-decreasing from 0 in steps of 1.
 * plain = arg-max of the sampled logits, merged = arg-max over the merged classes of the
 * per-class maximum, restricted = arg-max within the merged class `label`, first maximum on
 * ties (logits are taken to be finite: a NaN never wins here, while torch's arg-max
 * returns it).  soft = merged == label || label >= open_from; det = !soft; with is_last, entry 0 of
 * the last camera (if it has one) is set in both.
 *
 * veon_align_select_emit.  With score (K2,n_kept) (veon_occ_retrieve's cosines at `voxels`
 * against the K2 class rows) and table_norms (K2) given, the stage-2 rule first clears the
 * soft bit of entry i when score[k*] >= thr and priority[pred] > priority[merged_i], k* =
 * arg-max_k score[k] * table_norms[k] and pred the merged arg-max of the same products;
 * result counts such entries per camera as ignored.  score NULL: no stage 2.  Then, per
 * term (det by label, soft by merged class), with count = entries of the class in the
 * camera, norm = sum of priority over the classes present in the camera, per_cam and total
 * the entries of the camera and of all cameras:
 *   weight = 1 / count [* priority[class], soft only] / norm * (per_cam / max(total, 1))
 *            [* det_scale, det only] / batch_size
 * out_voxels (3 ints), out_labels (restricted for det, plain for soft) and out_weights hold
 * the det entries first, then the soft entries, each in kept order; `capacity` entries
 * (n_kept + 1 suffices: only the forced entry is in both).  result (2 + 3 n_cam ints):
 * n_det, n_soft, det per camera, soft per camera, ignored per camera.  Workspaces: totals
 * (2 * ceil(n_kept / 256) ints), norms (4 n_cam floats), head as _mark left it. */
int64_t veon_align_select_groups(int n_cam, int Xo, int Yo, int Zo);
int veon_align_select_mark(const void *labels, int labels_are_int64, int n_cls,
                           const float *cams, int n_cam, int Xo, int Yo, int Zo,
                           const float *grid, unsigned long long *masks, int *offsets,
                           int *head, int n_head, void *stream);
int veon_align_select_classify(const void *labels, int labels_are_int64, int n_cls,
                               const float *cams, int n_cam, int Xo, int Yo, int Zo,
                               const float *grid, const unsigned long long *masks,
                               const int *offsets, int *head, const float *sem, int K2,
                               int hs, int ws, float half_w, float half_h, const int *gid,
                               int open_from, int n_kept, int is_last, int *pair,
                               int *voxels, int *classes, int *flags, void *stream);
int veon_align_select_emit(const int *pair, const int *voxels, const int *classes,
                           int *flags, int n_kept, int n_cam, int n_vox, int n_cls,
                           const float *score, const float *table_norms, int K2,
                           const int *gid, float thr, const float *priority,
                           float det_scale, int batch_size, int *head, int n_head,
                           int *totals, float *norms, int *result, int capacity,
                           int *out_voxels, int *out_labels, float *out_weights,
                           void *stream);

/* ======== depth_loss.hip ============================================================ */

/* Depth pre-training loss, VeonDepthPretrain.forward_train
 * (detectors/veon_depth_pretrain.py:128-154): downsample_depth of the prediction (by sp)
 * and of the LiDAR depth (by sg), the mean-absolute-error statistic and
 * get_depth_loss_own(zoe, ce) (necks/view_transformer_raw.py:497-535), forward and
 * backward, with no read-back, no atomics and no memset.  depth (BN,Hp,Wp) and gt_depth
 * (BN,Hg,Wg) fp32 contiguous; sp, sg in {1, 2, 4, 8, 16}, each dividing its map, and
 * Hp/sp = Hg/sg = h, Wp/sp = Wg/sg = w, otherwise VEON_ERR_BAD_ARG.  A row is one of the
 * BN*h*w output pixels (at most 2^31 - 1); 1 <= D <= 32767; rec is 16-byte aligned.
 *
 * veon_depth_loss_rows writes one record of VEON_DEPTH_LOSS_REC floats per row, with
 * d / t the block-min of the row's prediction / label block, zeros read as 1e5:
 *   [0] g = log(d + 1e-7) - log(t + 1e-7)      [4] d
 *   [1] |d - t|                                [5] t
 *   [2] two-hot BCE of the row, 0 unless fg    [6] d [2] / d d, 0 unless fg
 *   [3] int: bit 0 valid (t < 9225),           [7] int: bits 0-7 the winning pixel
 *       bit 1 fg (label bin k* < D)                dy*sp + dx (first on ties), bit 8 set
 *                                                  when it was a zero, bits 16-30 k*
 * k* = argmax_k -|min(t, 500) - c_k| (first on ties) over the D+1 centres
 * c_k = k*step + (lo + step/2) of veon_two_hot_depth; [2] = -log p_k* - sum_{k<D, k!=k*}
 * log(1 - p_k), logs clamped at -100, p the softmax of -gamma*|d - c_k| clamped at -16.
 * [6] is autograd's: the clamp is straight-through (slope -gamma*sign(d - c_k) on every
 * bin) and binary_cross_entropy's backward is (p - y)/max(p(1 - p), 1e-12).
 *
 * veon_depth_loss_reduce (one workgroup, fixed-order fp64 sums) writes
 *   out[0] = min(sqrt(Dg), 2), Dg = var(g) + 0.15 mean(g)^2 over the n valid rows
 *            (unbiased; n < 2 gives NaN as the torch formulation does)
 *   out[1] = 0.05 * sum of [2] / max(1, n_fg)      out[2] = mean [1] over the valid rows
 *   coef[0..7] = mean, a = 1/((n-1) sqrt Dg), b = 0.15 mean/(n sqrt Dg) (a = b = 0 when
 *            clipped), 0.05/max(1, n_fg), n, n_fg, sqrt Dg, 1.0 when clipped.
 *
 * veon_depth_loss_bwd stores EVERY element of grad (BN,Hp,Wp): on a row's winning pixel,
 * unless that pixel was a zero,
 *   *g_zoe * ((g - mean) a + b)/(d + 1e-7)  [valid rows]  +  *g_ce * coef[3] * [6]  [fg]
 * and 0 elsewhere.  g_zoe / g_ce: device scalars, NULL = that loss has no gradient. */
#define VEON_DEPTH_LOSS_REC 8
int veon_depth_loss_rows(int BN, int Hp, int Wp, int sp, int Hg, int Wg, int sg, int D,
                         float lo, float step, float gamma, const float *depth,
                         const float *gt_depth, float *rec, void *stream);
int veon_depth_loss_reduce(int64_t rows, const float *rec, float *out, float *coef,
                           void *stream);
int veon_depth_loss_bwd(int BN, int Hp, int Wp, int sp, const float *rec, const float *coef,
                        const float *g_zoe, const float *g_ce, float *grad, void *stream);

/* ======== lidar_depth.hip =========================================================== */

/* The LiDAR depth labels of the depth pre-training stage, PointToMultiViewDepth
 * (datasets/pipelines/loading.py:735-759 points2depthmap, :811-821 the projection), as the
 * exact minimum kept depth per pixel, or per block x block pixels.
 * points (B,P,row_stride) fp32, row_stride >= 3 floats, the first three of a row are read;
 * lidar2img (B,N,3,4) fp32 (rows R | t of the 4x4's upper three), post_rots (B,N,3,3),
 * post_trans (B,N,3); out (B,N,H/block,W/block) fp32, all contiguous.  H x W is the map
 * AFTER `downsample`; block in {1, 2, 4, 8, 16} divides both; 0 < lo < hi; 1 <= B <= 65535,
 * B*P <= 2^31 - 1, H, W <= 2^24; otherwise VEON_ERR_BAD_ARG.  P = 0 is allowed.
 *
 * Per point and camera, fp32, one rounding per operation in this order:
 *   q = (R p) + t;  (u, v, d) = post_rot (q.x / q.z, q.y / q.z, q.z) + post_tran
 *   x = rint(u / downsample), y = rint(v / downsample)   (round-half-to-even: torch.round)
 *   kept iff x >= 0, x < W, y >= 0, y < H, d < hi, d >= lo, all tested in floating point:
 *   NaN, infinities, q.z = 0 and huge coordinates fail a comparison; x = -0.0 is pixel 0.
 * lidar2img == NULL: the rows are image points (u, v, d) already (points2depthmap alone),
 * post_rots / post_trans are not read and N must be 1.
 *
 * out[b][n][y / block][x / block] = the smallest kept d, 0 where nothing landed.  Kept
 * depths are positive, so their bit patterns order as their values: an unsigned atomic
 * minimum on out's own storage, exact and independent of the point order (repeated calls
 * and permuted points give the same bits).  EVERY element of out is written; no workspace,
 * no read-back, three launches (two when P = 0) on `stream`, capturable.  For hi <= 1e5
 * the block result equals downsample_depth(block = 1 result, block) with that function's
 * 1e5 for an empty block read as 0, bit for bit. */
int veon_lidar_depth_render(const float *points, int B, int P, int row_stride,
                            const float *lidar2img, const float *post_rots,
                            const float *post_trans, int N, int H, int W, int downsample,
                            int block, float lo, float hi, float *out, void *stream);

/* ======== image_inputs.hip ========================================================== */

/* The camera inputs of the pipeline step PrepareImageInputs (datasets/pipelines/
 * loading.py:1073-1329) from decoded frames: Pillow's 8-bit bicubic Image.resize bit for
 * bit, the crop window, the optional column mirror, the normalised planes, and the
 * depthanythingv2 tail of the depth branch.  All tensors contiguous.
 *
 * Resampling tables of one axis, in -> out (veon_amd/image_inputs.py resize_coeffs, Pillow's
 * precompute_coeffs + normalize_coeffs_8bpc): bounds (out,2) int32 = first tap and tap count
 * of each output index, kk (out,ksize) int32 = the coefficients in 22-bit fixed point.  One
 * pass is  ss = 2^21 + sum_t pixel[first + t] * kk[t];  out = clamp(ss >> 22, 0, 255)  in
 * 32-bit integers.  The kernels clamp first / count to the source extent, so a wrong table
 * cannot make them read outside it.  BN, rows, fH, oh in 1 .. 65535. */

#define VEON_IMAGE_MAX_WINDOWS 32

/* Window origins inside the resized image and column mirrors, by value: image bn of a call
 * uses entry bn % n (n = 1: one window for all; n = N: one per camera of every sample). */
typedef struct veon_image_windows {
  int n;
  int x0[VEON_IMAGE_MAX_WINDOWS];
  int y0[VEON_IMAGE_MAX_WINDOWS];
  int flip[VEON_IMAGE_MAX_WINDOWS];
} veon_image_windows;

/* Horizontal pass of source rows row0 .. row0 + rows - 1 only (the rows the vertical pass of
 * the windows reads): frames (BN,H,W,3) uint8 -> tmp (BN,rows,Wo,3) uint8. */
int veon_image_resample_h(const uint8_t *frames, int BN, int H, int W, int Wo, int row0,
                          int rows, const int *bounds, const int *kk, int ksize,
                          uint8_t *tmp, void *stream);

/* Vertical pass on the windows and the finish.  src (BN,Hs,Ws,3) uint8 holds rows
 * row0 .. row0 + Hs - 1 of the horizontally resized image (tmp above, or the frames
 * themselves with row0 = 0 when the width does not change); Ho is the resized height and
 * bounds / kk its tables (Ho rows).  bounds == NULL: no vertical pass (a pass whose size
 * does not change is skipped, as in Pillow): window row y is source row y0 + y.
 * Window pixel (y, x) of image bn is resized pixel (y0 + y, x0 + (flip ? fW - 1 - x : x)).
 * Writes either or both of
 *   canvas (BN,fH,fW,3) uint8: the transformed image (the reference's `canvas`);
 *   planes (BN,3,fH,fW) fp32:  planes[c] = lut[c][canvas[..., swap ? 2 - c : c]], lut
 *                              (3,256) fp32 on the device (the reference's normalisation
 *                              is a function of a byte; the host tabulates it).
 * A window outside the resized image (or outside src when bounds == NULL), n outside
 * 1 .. 32, both outputs NULL: VEON_ERR_BAD_ARG.  Every element of the outputs given is
 * written; one launch, no workspace, capturable. */
int veon_image_resample_v_finish(const uint8_t *src, int BN, int Hs, int Ws, int row0,
                                 int Ho, const int *bounds, const int *kk, int ksize,
                                 veon_image_windows win, int fH, int fW, const float *lut,
                                 int swap, uint8_t *canvas, float *planes, void *stream);

/* depthanythingNormalize's tail (loading.py:1048-1069): src (BN,h,w,3) uint8 -> out
 * (BN,3,oh,ow) fp32.  Channel c reads src channel swap ? 2 - c : c; x = u / 255; cubic
 * resize by OpenCV's INTER_CUBIC rule as far as it is stated here:
 *   fx = (float)((dx + 0.5) * ((double)w / ow) - 0.5), sx = floor(fx), t = fx - sx, A = -0.75
 *   w0 = ((A (t+1) - 5A)(t+1) + 8A)(t+1) - 4A,  w1 = ((A+2) t - (A+3)) t t + 1,
 *   w2 = w1 at 1 - t,  w3 = 1 - w0 - w1 - w2;  taps sx - 1 .. sx + 2 clamped to the image;
 *   rows first (taps summed left to right), then columns;
 * then (x - mean[c]) / std[c].  fp32, one rounding per operation. */
int veon_image_cubic_norm(const uint8_t *src, int BN, int h, int w, int oh, int ow, int swap,
                          float mean0, float mean1, float mean2, float std0, float std1,
                          float std2, float *out, void *stream);

/* ======== occ_bin_loss.hip ========================================================== */

/* The occupancy term of the training loss, BCE_BinOcc_Loss
 * (loss/occ_loss_utils/occ3d_nuscenes.py:200-212) on the trilinearly upsampled bin_occ
 * (san_in_veon_temporal.py:202-210), from the LOW-resolution logits, forward and backward,
 * with no read-back, no atomics and no memset; the upsampled logits are never stored.
 * logits (B,2,zi,yi,xi) fp32 through five ELEMENT strides {b, c, z, y, x} (all >= 0);
 * labels (B,Xo,Yo,Zo) uint8 contiguous: output voxel (zo, yo, xo) has label
 * labels[b][xo][yo][zo]; class_weights: 2 floats (w_0, w_1) on the device.  B*Zo*Yo*Xo is
 * at most 2^31 - 1, otherwise VEON_ERR_BAD_ARG.
 *
 * With up = trilinear(logits, align_corners=False) at the output voxel (the index rule of
 * occ_align_loss.hip and occ_retrieval.hip), t = 0 for label < free_index and 1 for
 * label >= free_index, and voxels with label == ignore_index not counted:
 *   nll   = logsumexp(up_0, up_1) - up_t   (the maximum subtracted first)
 *   loss  = sum w_t nll / sum w_t          over the counted voxels
 * veon_occ_bin_loss_fwd writes
 *   coef[n] = w_t (p_0 - [t == 0]) = d (w_t nll) / d up_0, 0 where ignored, one float per
 *             output voxel in LABEL order (n = ((b Xo + xo) Yo + yo) Zo + zo); the
 *             derivative with respect to up_1 is -coef[n]
 *   out[0]  = loss (NaN when every voxel is ignored, as torch)
 *   out[1]  = 1 / sum w_t (0 when every voxel is ignored: the gradient is then all zeros)
 * `workspace`: veon_occ_bin_loss_workspace_bytes(B, Zo, Yo, Xo) bytes (host-only; -1:
 * unsupported size), 8-byte aligned: per-workgroup fp64 partial sums, added in a fixed
 * order; too small gives VEON_ERR_WORKSPACE.  Repeated calls are bit-identical.
 *
 * veon_occ_bin_loss_bwd, for the grid (2 zi, 2 yi, 2 xi) only: stores EVERY element of
 * grad (B,2,zi,yi,xi) fp32 contiguous,
 *   grad[b][0][i] = *gout * out[1] * sum over the outputs o that read i of coef[o] *
 *                   (product of the three axis weights with which o reads i),
 *   grad[b][1][i] = -grad[b][0][i],
 * the outputs visited in a fixed order ([2i-1, 2i+2] per axis, clipped to the grid; the
 * weights come from the forward's own index rule, clamped borders included).  coef and out
 * as the forward wrote them for that grid; gout: the upstream gradient, a device scalar. */
int64_t veon_occ_bin_loss_workspace_bytes(int B, int Zo, int Yo, int Xo);
int veon_occ_bin_loss_fwd(const float *logits, const int64_t *logit_strides, int B, int zi,
                          int yi, int xi, int Zo, int Yo, int Xo,
                          const unsigned char *labels, const float *class_weights,
                          int ignore_index, int free_index, float *coef, void *workspace,
                          int64_t workspace_bytes, float *out, void *stream);
int veon_occ_bin_loss_bwd(const float *coef, const float *out, const float *gout, int B,
                          int zi, int yi, int xi, float *grad, void *stream);

/* ======== fusion_train.hip ========================================================== */

/*
 * ---- training of the lift's 2-D fusion (CatFusionLift, semantic_net/layers.py:154-199)
 * on token rows ----
 * x (N, Cin, Hin, Win) is an fp32 NCHW map, contiguous; the lift's map is H x W, M = N*H*W
 * tokens; rc / drc are fp32 rows [M][C] and the map owns their columns coff .. coff + Cin.
 * The filter is torch's bilinear resize (align_corners = False, no antialias) read from
 * per-axis tables the host computes in fp32 once per shape pair (taby: Hin -> H, tabx:
 * Win -> W).  A table of `in` source and `out` destination positions is 3 * out + 2 * in
 * 32-bit words on the device, 16-byte aligned:
 *     i0[out] | i1[out] | l1[out] (float) | first[in] | last[in]
 * src = max((d + 0.5f) * ((float)in / out) - 0.5f, 0) with the multiply-subtract rounded
 * once (torch's kernels contract it), i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0;
 * source s is read by the destinations first[s] <= d < last[s] (i0 is monotone: one range).  Indices read from a table are clamped to their
 * axis.  A map already at H x W is copied (weights 1 and 0) and takes no tables (NULL).
 * Cin % 64 == 0, C % 4 == 0, coff % 4 == 0, every tensor below 2^31 elements and
 * N * max(H, Hin) <= 65535, otherwise VEON_ERR_BAD_ARG.
 *
 * veon_fusion_resize_cat     : rc[:, coff : coff + Cin] = resize(x), channels-last.
 * veon_fusion_resize_adjoint : dx = resize^T(drc[:, coff : coff + Cin]) in gather form:
 *                              every source pixel adds the tokens whose footprint holds it
 *                              in index order; a pixel no token reads is written as ZERO.
 *                              No atomics, no cleared output, bit-reproducible.
 */
int veon_fusion_resize_cat(const float *x, float *rc, const void *taby, const void *tabx,
                           int N, int Cin, int Hin, int Win, int H, int W, int C, int coff,
                           void *stream);
int veon_fusion_resize_adjoint(const float *drc, float *dx, const void *taby,
                               const void *tabx, int N, int Cin, int Hin, int Win, int H,
                               int W, int C, int coff, void *stream);

/*
 * Both LayerNorms of the module from one read of a row: xn1 half [M][C1 + C2] =
 * LN1(rc), xn2 half [M][C2] = LN2(rc[:, C1:]); biased variance, eps inside the sqrt,
 * two-pass statistics from registers, one wave per row.
 * C1 % 64 == 0, C2 % 64 == 0, C1 + C2 <= 2048, M * (C1 + C2) < 2^31.
 */
int veon_fusion_dual_ln(const float *rc, const float *gamma1, const float *beta1,
                        const float *gamma2, const float *beta2, void *xn1, void *xn2, int M,
                        int C1, int C2, float eps1, float eps2, void *stream);

/*
 * Their backward at the stored fp32 rows rc (statistics recomputed): dxn1 half
 * [M][C1 + C2], dxn2 half [M][C2] -> drc fp32 [M][C1 + C2], whose columns from C1 on are
 * the sum of both branches, and sums fp32 [2 (C1 + C2) + 2 C2] =
 * dgamma1 | dbeta1 | dgamma2 | dbeta2.  Two stages in a fixed order, no atomics;
 * `workspace`: veon_fusion_dual_ln_bwd_workspace_bytes(C1, C2) bytes (host-only; -1:
 * unsupported widths).  Widths as veon_fusion_dual_ln.  drc must not alias rc.
 */
int64_t veon_fusion_dual_ln_bwd_workspace_bytes(int C1, int C2);
int veon_fusion_dual_ln_bwd(const void *dxn1, const void *dxn2, const float *rc,
                            const float *gamma1, const float *gamma2, float *drc,
                            float *sums, void *workspace, int64_t workspace_bytes, int M,
                            int C1, int C2, float eps1, float eps2, void *stream);

/*
 * Around the ReLU.  y1 half [M][ld1], y2 half [M][ld2] are the GEMM outputs (bias and
 * ReLU applied by the GEMM's epilogue), of which the first p1 / p2 columns count.
 * veon_fusion_join       : out fp32 [M][p1 + p2] = cat(y1[:, :p1], y2[:, :p2]).
 * veon_fusion_relu_split : dy1 half [M][ld1], dy2 half [M][ld2] = the columns of dout
 *                          fp32 [M][p1 + p2] where the stored output is positive, zero
 *                          elsewhere and in the padding columns.
 * p1 % 4 == 0, p2 % 4 == 0, ld % 8 == 0, ld >= p, M * (ld1 + ld2) < 2^31.
 */
int veon_fusion_join(const void *y1, const void *y2, float *out, int M, int p1, int p2,
                     int ld1, int ld2, void *stream);
int veon_fusion_relu_split(const float *dout, const void *y1, const void *y2, void *dy1,
                           void *dy2, int M, int p1, int p2, int ld1, int ld2,
                           void *stream);

/* ======== volume_handover.hip ======================================================= */

/* Hand-over between the padded half rows the prediction heads train on and the fp32
 * channels-last tensors of the feature-alignment loss.
 *
 * veon_volume_unpack_cl_f32: interior of a padded half grid [B][Z+2][Y+2][X+2][Cp] -> out
 * (B,Z,Y,X,C) fp32 contiguous (16-byte aligned), the first C <= Cp channels; Cp % 4 == 0.
 *
 * veon_volume_sigm_bwd_pack_cl: backward of f = sigmoid(pre) - 0.5 fused with the pack.
 * grad: fp32 (B,Z,Y,X,C) through four ELEMENT strides {b, z, y, x} (all >= 0, x stride
 * >= C), channel stride 1; f_storage / out_storage: whole storages of padded half grids
 * of C channels, guard_rows = veon_conv3d_guard_rows(Y, X) rows before and after the
 * padded rows (anything else is VEON_ERR_BAD_ARG), C % 4 == 0, not aliased.  Every row
 * of out_storage is stored: d pre = grad * (0.25 - f^2) rounded to half on interior
 * rows, ZERO on halo and guard rows (no memset needed). */
int veon_volume_unpack_cl_f32(const void *padded, float *out, int B, int Cp, int C, int Z,
                              int Y, int X, void *stream);
int veon_volume_sigm_bwd_pack_cl(const float *grad, const int64_t *grad_strides,
                                 const void *f_storage, void *out_storage,
                                 int64_t guard_rows, int B, int C, int Z, int Y, int X,
                                 void *stream);

/* ======== optim_step.hip ============================================================ */

/* The parameter update of a training iteration: clip_grad_norm_(max_norm, norm_type = 2),
 * AdamW (the configs under configs/veon: lr 1e-4, weight_decay 1e-2, grad_clip max_norm 5) and the
 * weight EMA of MEGVIIEMAHook (mmdet3d/core/hook/ema.py:48-59) over flat fp32 arenas.
 * fp32 only; no atomics, no read-back, no allocation, every call bit-reproducible.
 *
 * The gradients, exp_avg and exp_avg_sq of every trained tensor live at the same element
 * offset of three arenas of n floats, n a multiple of veon_optim_chunk() (4096), each
 * tensor's slot starting at a multiple of 4 elements, padding zero, bases 16-byte aligned.
 *
 * veon_optim_sumsq: partials[c] = sum of squares of chunk c of grad (n / chunk partials),
 * in the fixed order csrc/optim_step.hip states.
 * veon_optim_clip_finish (one workgroup): adds the partials in fp64 in a fixed order,
 *   scal[0] = norm = fp32(sqrt(sum)),  scal[1] = coef = min(max_norm / (norm + 1e-6f), 1)
 * where a NaN stays NaN (clip_grad_norm_ with error_if_nonfinite=False); max_norm > 0.
 *
 * veon_optim_update: one workgroup per record (the grid is capped and strides).  A record
 * is at most one chunk of one tensor: p and ema point at the piece's first element, offset
 * is its element offset in the arenas, count its length (1 .. chunk), group its row of the
 * per-group scalars.  ema == NULL: no EMA of this piece.  offset == -1: EMA-only (a buffer
 * or a frozen parameter; p is only read).  16-byte accesses where p and ema are 16-byte
 * aligned, element accesses otherwise.  The table is on the device.  scal: the buffer of
 * veon_optim_clip_finish, or NULL for coef = 1.  host_scalars: HOST doubles, rounded to fp32
 * here: {c_d, c_1md} and then VEON_OPTIM_GROUP_SCALARS per group, {c_decay, c_1mb1, c_b2,
 * c_1mb2, c_step, c_bc2, c_eps}; n_groups <= VEON_OPTIM_MAX_GROUPS (0: grad, exp_avg and
 * exp_avg_sq may be NULL and every record must be EMA-only).  Per element, in this order:
 *   g = grad * coef
 *   p = p * c_decay                                 c_decay = 1 - lr * weight_decay
 *   m = m + c_1mb1 * (g - m)                        c_1mb1  = 1 - beta1
 *   v = v * c_b2 + c_1mb2 * (g * g)                 c_b2 = beta2, c_1mb2 = 1 - beta2
 *   p = p - c_step * (m / (sqrtf(v) / c_bc2 + c_eps))
 *                                  c_step = lr / (1 - beta1^t), c_bc2 = sqrt(1 - beta2^t)
 *   e = e * c_d + c_1md * p                         c_d = d, c_1md = 1.0 - d
 * The clipped gradient is not stored: nothing reads it before the next zero_grad.  The
 * per-step scalars are launch arguments, so a captured graph would replay one step's
 * values: the step is launched, not replayed. */
#define VEON_OPTIM_MAX_GROUPS 8
#define VEON_OPTIM_GROUP_SCALARS 7
typedef struct veon_optim_record {
  float *p;
  float *ema;
  int64_t offset;
  int32_t count;
  int32_t group;
} veon_optim_record;
int veon_optim_chunk(void);
int veon_optim_sumsq(const float *grad, int64_t n, float *partials, void *stream);
int veon_optim_clip_finish(const float *partials, int64_t n_partials, double max_norm,
                           float *scal, void *stream);
int veon_optim_update(const veon_optim_record *records, int64_t n_records,
                      const float *grad, float *exp_avg, float *exp_avg_sq,
                      const float *scal, const double *host_scalars, int n_groups,
                      void *stream);

/* ======== sem2d.hip ================================================================= */

/* The semantic tail of SAN's 2-D branch (mmdet3d/models/semantic_net/
 * san_in_veon_temporal.py:176-186, 240-255): cls = softmax(mask_logits)[..., :-1] and the
 * mask embeddings spread over the sigmoid of the Q mask proposals.  All tensors fp32 and
 * contiguous: mask_logits (B,Q,K+1), mask_embs (B,Q,C), mask_preds (B,Q,h,w).  probs: a
 * workspace of B*Q*K floats that receives cls (the only workspace; written by every
 * call, so calls on one stream may share it).  Q <= 256, K + 1 <= 256, B <= 65535,
 * h * w < 2^23, otherwise VEON_ERR_BAD_ARG.  Every sum over q runs in index order with one
 * fmaf per term: no atomics, no memset, every output element written, repeated calls
 * bit-identical.  +-inf in mask_preds is undefined (NaN propagates as in torch).
 *
 * veon_sem2d_ds (san_in_veon_temporal.py:176, 248-255): sem_seg_ds (B,K,h,w) and, with
 * mask_embs, sem_embed_ds (B,C,h,w); mask_embs and sem_embed_ds are given or NULL
 * together. */
int veon_sem2d_ds(const float *mask_logits, const float *mask_embs, const float *mask_preds,
                  int B, int Q, int K, int C, int h, int w, float *probs, float *sem_seg_ds,
                  float *sem_embed_ds, void *stream);
/* veon_sem2d_full (san_in_veon_temporal.py:179-185, 240-246): sem_seg (B,K,H,W) =
 * sum_q cls * sigmoid(bilinear(mask_preds)) with ATen's align_corners=False arithmetic
 * (scale = in / out in float, src = max(scale * (dst + 0.5) - 0.5, 0), upper tap clamped
 * to the last pixel); any positive h, w, H, W with H <= 262140.  The (B,Q,H,W) tensor
 * is never formed. */
int veon_sem2d_full(const float *mask_logits, const float *mask_preds, int B, int Q, int K,
                    int h, int w, int H, int W, float *probs, float *sem_seg, void *stream);
/* veon_sem2d_labels (san_in_veon_temporal.py:179-185, 240-246, then the arg-max a caller
 * takes): uint8 labels (B,H,W) of the values veon_sem2d_full writes (the same arithmetic,
 * bit for bit), and nothing else.  group (HOST, K bytes, or NULL): the merged channel of
 * every row as in veon_occ_labels_grouped, n_merged <= 64; each run of rows is merged by
 * its maximum.  The label is the lowest (merged) channel that attains the maximum; a
 * pixel with a NaN in any row gets ignore_label (0 .. 255). */
int veon_sem2d_labels(const float *mask_logits, const float *mask_preds, int B, int Q, int K,
                      int h, int w, int H, int W, const uint8_t *group, int n_merged,
                      int ignore_label, float *probs, uint8_t *labels, void *stream);

/* ======== memory.hip ================================================================ */

/* Physically contiguous device memory (hipExtMallocWithFlags +
 * hipDeviceMallocContiguous) for the lift's output volume, whose write pattern
 * (C planes 4*Z*Y*X bytes apart per workgroup) is sensitive to the page-table
 * fragment size; VEON_ERR_LAUNCH when the driver cannot provide it (the caller
 * then keeps an ordinary allocation).  No reference counterpart: the reference
 * lets torch.zeros allocate the volume (bev_pool.py:17-19). */
int veon_alloc_contiguous(void **ptr, int64_t bytes);
/* the same with any hipExtMallocWithFlags flag (probe tool) */
int veon_alloc_device_flags(void **ptr, int64_t bytes, unsigned flags);
int veon_free_device(void *ptr);

/* ======== experiment setters ======================================================== */
/* Knobs of the tools and of the tile-forcing tests, defined in bev_pool_rows.hip,
 * vit_block.hip and conv3d.hip; the product path never calls them. */

/* experiment knob of tools/poolbench.py / tools/xcd_order_ab.py; 0 = production.
 * bits 0-3: ablations of the row max-pool kernel (results invalid); bit 4: tile =
 * blockIdx instead of the XCD-grouped tile order; bits 8-11: (lg + 1) forces runs of
 * 2^lg tiles per XCD -- the order never changes a result. */
void veon_pool_debug_set(int flags);
/* tuning knobs of the row max-pool kernel (0 = built-in default): worker
 * workgroups, longest cold list, longest warm list */
void veon_pool_tune_set(int workers, int cold_max, int warm_max);

/* experiment knob of tools/gemm_bench.py: force the tile configuration of
 * veon_vit_gemm (-1 = automatic, 0 = small-tile kernel, 1..6 = ring-kernel tiles) */
void veon_gemm_ring_set(int config);
/* Force the small-tile kernel's shape (wm waves down, wn across, mt 16-row blocks per
 * wave) of veon_vit_gemm when it takes that kernel (veon_gemm_ring_set(0) sends every
 * shape there); overrides the VEON_GEMM_SMALL=wm,wn,mt knob of tools/gemm_bench.py.
 * Instantiated: (4,2,1) (4,2,2) (4,4,1) (4,4,2) (8,2,1); any other triple returns
 * VEON_ERR_BAD_ARG and changes nothing.  wm = -1: back to automatic. */
int veon_gemm_small_set(int wm, int wn, int mt);

/* experiment knob of tools/body_bench.py (ablations of the conv kernels' loads;
 * non-zero flags give WRONG results): 0 = normal.  Correct-result bits: 8 (bit 3) takes
 * the general kernel instead of the slab-sharing one; bits 16..27 force the tile (wm, wn,
 * mt: four bits each) -- while they name a tile that is not instantiated, the conv
 * entry points return VEON_ERR_BAD_ARG. */
void veon_conv_debug_set(int flags);

#ifdef __cplusplus
}
#endif
#endif /* VEON_HIP_H_ */
