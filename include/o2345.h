/* o2345.h -- C ABI of libo2345_hip.so: the MI355X (gfx950) reconstruction back end for One-2-3-45.
 *
 * Drop-in boundary: the reference has no native code of its own; its hot path reaches native kernels
 * only through three un-vendored pip packages (torchsparse v1.4.0, inplace_abn, PyMCubes) and ATen.  This header is
 * what a binding for that path links against; the Python shims in one-2-3-45_amd/ (ctypes) expose
 * the reference's own Python operator surface on top of it.  Every entry cites the reference interface it replaces
 * (paths relative to /root/reference/reconstruction).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / C++ types.  A pointer is a HOST pointer if and only if its name
 *     ends in _host, or the function's name ends in _host; every other pointer, a struct's fields among them, is a
 *     DEVICE pointer.  A binding reads this, and every pointer's element type, from the declarations below
 *     (one-2-3-45_amd/_lib.py does).  The caller owns every buffer; the library never allocates, frees or retains them.
 *   - every struct that crosses this boundary is declared below, once (typedef struct O2345...): csrc/ compiles that declaration, a binding
 *     generates its own from the same text and checks it against o2345_struct_size / o2345_struct_layout of the loaded library.
 *   - every function returns 0 on success, a negative code on error; o2345_last_error() (thread-local) explains.
 *   - `stream` is a hipStream_t (NULL = default stream).  Functions are asynchronous unless stated otherwise and
 *     re-entrant (one Python thread per device under nn.DataParallel is fine).
 *   - all arithmetic is fp32 (fp64 for batch-norm statistics and marching-cubes vertices), voxel / row ids int32.
 *   - variable-size outputs: capacity buffer + device-side count (cost volume, sparse levels) or the two-call
 *     count -> emit protocol (marching cubes).
 *   - no process-global state: nothing is retained between calls except, per library instance, the O2345_* debug knobs (read once, o2345_knobs())
 *     and which kernels had their LDS limit raised on which device.  One host thread per stream / device; several streams may share a GPU.
 *
 * Accuracy contract (HIP vs the reference's arithmetic as restated by oracle/, which is pinned to reference-generated golden vectors)
 *   - exact: kept-voxel set, visible-view counts, sparse level coordinates, nearest-mask lookups, valid-view counts and colour masks, list contents,
 *     marching-cubes triangles for an identical scalar field; results do not depend on batch composition (chunked == one call, bit for bit) or on
 *     which of the two sampler kernel forms runs.
 *   - per stage, max abs error relative to max(1, |reference|): cost-volume rows 2e-5 (1.3e-4 at 128^3: var = E[x^2] - mean^2 cancels), sparse CNN and
 *     dense volume 3.5e-5, SDF 2e-6, SDF gradient 1e-5, new sample depths 2e-4 and 5e-3 of their bin, compositing on identical sample lists colour 3e-5,
 *     depth / weights / depth variance 2e-5.  Both numerical modes (O2345RenderIO.sdf_mode 2 = split-f16 on the matrix cores, 0 = fp32 MFMA) meet the same bounds.
 *   - end to end through render(): the reference's hierarchical sampler amplifies fp32-class SDF differences (sigmoid slopes 64 ... 512, inverse CDF over
 *     nearly empty bins), so the bound is distributional: sample lists within one coarse section, rays with coinciding lists as tight as the stage bound,
 *     and at BASELINE config 2 colour error max <= 6e-2 (measured 4.2e-2), q99 <= 8e-3 (3.1e-3), <= 6 % of the rays above 1e-3 (2.2 %) -- within 4x what
 *     the reference itself does under 1e-6 SDF noise.  Mesh: a lattice node may change sign only where |u| <= 9e-7 (0 - 1 node of 262,144), sizes equal, IoU >= 0.999.
 *   - unpinned (no source in the reference tree): inplace_abn's |gamma| + eps, torchsparse v1.4.0's kernel maps, PyMCubes' vertex numbering.
 */
#ifndef O2345_H
#define O2345_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

const char* o2345_last_error(void);
/* 200 = ABI 2.0 (round 4): O2345RenderIO re-laid out (sdf_mode replaces the fossil name sdf_bf16; color_blob / the VALU colour kernel removed;
 * per-ray near / far; caller-owned colour work counters; per-call scalars) and layout-checked (o2345_render_io_*), o2345_camera_terms,
 * `identity_rows` on o2345_sparse_conv3d_x3, no process-global state left in the library (the colour work counters are a caller-owned buffer). */
/* 210 = ABI 2.1 (round 5): O2345RenderIO gains `segment_rays` (the reference's two per-CALL rules applied per segment of a fused call: a whole image
 * behind the trainer's unchanged 512-ray chunk loop) and `weight_cull` (tolerance-bounded colour work removal); o2345_ray_composite is unchanged.
 * Additive since 2.1 (no existing entry changed, the version stays 210): the asset export entries o2345_mesh_bounds_workspace_bytes,
 * o2345_mesh_asset_vertices, o2345_mesh_asset_indices, o2345_obj_text_bytes, o2345_obj_text, o2345_obj_text_host; the mesh component entries
 * o2345_mesh_components_workspace_bytes, o2345_mesh_components_count, o2345_mesh_components_emit; the adjacency and smoothing entries
 * o2345_mesh_adjacency_workspace_bytes, o2345_mesh_adjacency_count, o2345_mesh_adjacency_emit, o2345_mesh_smooth; the decimation entries
 * o2345_mesh_decimate_workspace_bytes, o2345_mesh_decimate_count, o2345_mesh_decimate_emit; the projection entries
 * o2345_mesh_project_workspace_bytes, o2345_mesh_project; the sparse lattice entries o2345_sdf_grid_sparse_workspace_bytes,
 * o2345_sdf_grid_sparse_x3; the mesh distance entries o2345_mesh_samples_workspace_bytes, o2345_mesh_samples_count, o2345_mesh_samples_emit,
 * o2345_mesh_distance_grid_workspace_bytes, o2345_mesh_distance_grid_bytes, o2345_mesh_distance_grid_count, o2345_mesh_distance_grid_emit,
 * o2345_mesh_distance_query, o2345_mesh_distance_reduce_workspace_bytes, o2345_mesh_distance_reduce. */
/* 220 = ABI 2.2: the four device stats blocks are declared structs (O2345ProjectStats, O2345TextureStats, O2345SurfaceStats, O2345DistanceStats; no byte
 * of them moved, the untyped `stats` parameters became pointers to them); o2345_struct_size / o2345_struct_layout describe every declared struct and replace
 * o2345_render_io_size / o2345_render_io_layout; the parameter of o2345_render_rays is called io_host. */
/* 230 = ABI 2.3: the stats blocks of the simplification and of the audit are declared structs too (O2345SimplifyStats, O2345AuditStats; no byte of them
 * moved, the `long long* stats` parameters became pointers to them); the positional enumerators that named their entries (O2345_SIMPLIFY_ROUNDS ... _STATS,
 * O2345_AUDIT_*) are removed, the three stop codes O2345_SIMPLIFY_STOPPED_* stay.  Both units were additive since 2.2: the simplification entries
 * o2345_mesh_simplify_workspace_bytes, o2345_mesh_simplify_count, o2345_mesh_simplify_emit; the audit entries o2345_mesh_audit_workspace_bytes,
 * o2345_mesh_audit.
 * Additive since 2.3 (no existing entry changed, the version stays 230): the hole-filling entries o2345_mesh_fill_workspace_bytes, o2345_mesh_fill_count,
 * o2345_mesh_fill_emit; the self-intersection entries o2345_mesh_intersect_workspace_bytes, o2345_mesh_intersect_count, o2345_mesh_intersect_emit; the
 * rasterizer entries o2345_mesh_raster_workspace_bytes, o2345_mesh_raster_count, o2345_mesh_raster_emit, o2345_mesh_raster_shade; the textured
 * shading entry o2345_mesh_raster_shade_textured. */
/* 231 = ABI 2.3.1: o2345_mesh_raster_count, o2345_mesh_raster_emit and o2345_mesh_raster_shade_textured take the camera as o2345_camera_rays does, K_host [9]
 * and c2w_host [12], in place of sixteen float scalars at the same position; nothing else changed.
 * Additive since 2.3.1 (no existing entry changed, the version stays 231): the mesh alignment entries o2345_mesh_align_workspace_bytes,
 * o2345_mesh_align_step; the ray cast entries o2345_mesh_ray_cast, o2345_mesh_occlusion. */
int o2345_version(void);
/* Layout self-description of the declared structs as THIS library was compiled (sizeof, and offsetof of every field in declaration order): a binding
 * asserts its own structs against it at load time (one-2-3-45_amd/_lib.py does) -- a field added on one side only cannot corrupt calls silently.
 * which: the struct's position among the `typedef struct O2345...` declarations of this header, from 0.  struct_layout writes min(n, number of fields)
 * offsets and returns the number of fields; both return 0 for a `which` out of range. */
size_t o2345_struct_size(int which);
int o2345_struct_layout(int which, size_t* offsets_host, int n);
/* The debug / A-B knobs this library instance runs with, e.g. "list_sort=1 sparse_brick=1 flat_sched=0 color_tiles=0 color_sched=10".  They are read from
 * the environment (O2345_LIST_SORT, O2345_SPARSE_BRICK, O2345_FLAT_SCHED, O2345_COLOR_KERNEL, O2345_COLOR_SCHED) ONCE, at the first call that needs
 * them -- this call included --, never on a launch path. */
const char* o2345_knobs(void);

/* ---- cost volume -------------------------------------------------------------------------------------------------
 * replaces: ops/generate_grids.py:4 generate_grid, ops/back_project.py:5 back_project_sparse_type (both calls),
 * models/sparse_sdf_network.py:221 aggregate_multiview_features, the frustum filter at :330-334.
 * proj: [V,4,4] row-major affine matrices (sample['affine_mats']); voxel (x,y,z) -> world = xyz*voxel_size + origin.
 * H and W, the height and width of the source images, are independent (each > 1; the reference's sizeH, sizeW): a projected x is normalised by W - 1, a
 * projected y by H - 1, maps are [V,H,W,C]; dx, dy, dz are independent too.  A voxel is seen by a view if |gx| <= 1, |gy| <= 1 and z > 0: the border of
 * the image counts.  (tests/test_gpu_project_units.py runs these entries at 28 x 44, 45 x 24 and 2 x 3.) */
size_t o2345_costvol_workspace_bytes(int dx, int dy, int dz);
/* visible-view count per voxel, order-preserving compaction of the voxels seen by > min_views views:
 * cnt [dx*dy*dz] u8, row_of_voxel [dx*dy*dz] (row id or -1), coords [capacity,4] int32 (x,y,z,batch=0), *n_rows_dev. */
int o2345_costvol_index(const float* proj, int V, int H, int W, int dx, int dy, int dz, float voxel_size,
                        const float* origin_host, int min_views, uint8_t* cnt, int32_t* row_of_voxel, int32_t* coords,
                        int32_t* n_rows_dev, void* workspace, size_t workspace_bytes, void* stream);
/* feats_nhwc [V,H,W,C] (C = 8|16) -> out_rows [n_rows, 2C] = cat(variance, mean) over the V views. */
int o2345_costvol_gather(const float* feats_nhwc, const float* proj, int V, int H, int W, int C, int dx, int dy, int dz,
                         float voxel_size, const float* origin_host, const uint8_t* cnt, const int32_t* coords,
                         int n_rows, float* out_rows, void* stream);
int o2345_nchw_to_nhwc(const float* in, float* out, int V, int C, int H, int W, void* stream);

/* ---- feature pyramid glue of FeatureNet (replaces the ATen kernels between its convolutions; ABI 1.2) ----------------------------------------
 * fpn_level: out [V,32,H,W] = 1x1 conv (weight [32,c_in], bias [32]) of fine [V,c_in,H,W] + bilinear x2 up-sampling (align_corners = True) of
 *   coarse [V,32,H/2,W/2]   (models/featurenet.py:73-76, 85-86: _upsample_add(feat, lat(conv))); c_in = 8 or 16.
 * pyramid_pack: the fused pyramid of models/trainer_generic.py:1117-1123 = [x4 up-sampled f2 (32) | x2 up-sampled s1 (16) | s0 (8)], written once:
 *   fmaps_nchw [V,56,H,W] (optional, may be NULL) and cmaps_nhwc64 [V,H,W,64] = rgb (3) | those 56 features | 5 zeros (the map the colour kernels
 *   gather from; replaces o2345_pack_color_maps on this path). */
int o2345_fpn_level(const float* fine, int c_in, const float* coarse, const float* weight, const float* bias, int V, int H, int W,
                    float* out, void* stream);
int o2345_pyramid_pack(const float* f2, const float* s1, const float* s0, const float* rgb, int V, int H, int W, float* fmaps_nchw,
                       float* cmaps_nhwc64, void* stream);
/* ---- the convolutions of FeatureNet and of the compress layer (ABI 1.3; replace nn.Conv2d + InPlaceABN pairs: models/featurenet.py:12-22
 * ConvBnReLU, :40-66 FeatureNet, models/sparse_sdf_network.py:171-173 compress_layer) ---------------------------------------------------------
 * conv2d: out [V,cout,Ho,Wo] = conv2d(act(in), w) (+ bias), padding k / 2, stride 1 or 2; w_packed = [cin][k][k][cout] (conv2d_pack_weights of an
 *   nn.Conv2d weight [cout,cin,k,k]).  in_scale_shift [2*cin] (may be NULL): the InPlaceABN of the PRODUCER of `in` is applied while `in` is read,
 *   act(x) = leaky_relu(x * scale + shift, slope) -- the activated tensor is never stored.  out_scale_shift [2*cout] (may be NULL): batch
 *   statistics of `out` over (V,Ho,Wo) -> this layer's own (scale, shift) = ((|gamma| + eps) / sqrt(var + eps), beta - mean * scale) for the
 *   consumer to apply (needs gamma, beta and a workspace of conv2d_workspace_bytes).  Shapes (fp32 form): the (cin, cout, k, stride) combinations of FeatureNet
 *   and the compress layer (16 or 8 outputs); anything else is an error.  The matrix-core form takes any cin <= 64, cout <= 32 with those (k, stride).
 * fpn_level_act: fpn_level whose `fine` input is a raw convolution output with its (scale, shift) applied on load.
 * scale_shift_act: y = leaky_relu(x * scale + shift) for x [V,C,H,W], written as NCHW and / or channel-last NHWC (C = 8, 16, 32). */
int o2345_conv2d_pack_weights(const float* w_oihw, int cout, int cin, int k, float* packed, void* stream);
size_t o2345_conv2d_workspace_bytes(int V, int cout, int Ho, int Wo);
int o2345_conv2d(const float* in, int V, int cin, int Hi, int Wi, int in_pixel_stride, int in_channel_offset, const float* in_scale_shift, float slope,
                 const float* w_packed, const float* bias, int cout, int k, int stride, float* out, const float* gamma, const float* beta, float eps,
                 int abs_gamma, float* out_scale_shift, void* workspace, size_t workspace_bytes, void* stream);
/* in_pixel_stride = 0: `in` is [V,cin,Hi,Wi] (channel-first).  in_pixel_stride > 0: `in` is a channel-last map [V,Hi,Wi,in_pixel_stride] and the
 * convolution reads its channels in_channel_offset .. + cin (the compress layer reads the 56 features of the [V,H,W,64] colour map at offset 3, so the
 * channel-first fused pyramid is never written on that path).
 * the same convolution on the matrix cores (split-f16 operands, fp32 accumulate: the default numerical mode); cin <= 64, cout <= 32;
 * w_packed_x3 [conv2d_x3_weight_floats] from conv2d_pack_weights_x3 */
size_t o2345_conv2d_x3_weight_floats(int cin, int k);
int o2345_conv2d_pack_weights_x3(const float* w_oihw, int cout, int cin, int k, float* packed, void* stream);
int o2345_conv2d_x3(const float* in, int V, int cin, int Hi, int Wi, int in_pixel_stride, int in_channel_offset, const float* in_scale_shift, float slope,
                    const float* w_packed_x3, const float* bias, int cout, int k, int stride, float* out, const float* gamma, const float* beta, float eps,
                    int abs_gamma, float* out_scale_shift, void* workspace, size_t workspace_bytes, void* stream);
int o2345_fpn_level_act(const float* fine, const float* fine_scale_shift, float slope, int c_in, const float* coarse, const float* weight,
                        const float* bias, int V, int H, int W, float* out, void* stream);
int o2345_scale_shift_act(const float* x, int V, int C, int H, int W, const float* scale_shift, float slope, float* y_nchw, float* y_nhwc,
                          void* stream);
/* lod > 0 (sparse_sdf_network.py:335-357): the same two passes for an explicit voxel list coords [n,4] (x,y,z,b) in arbitrary
 * order; cnt / cnt_row are per LIST ROW.  build_index_grid makes the dense row lookup of such a list (cells of size ts). */
int o2345_visible_count_list(const float* proj, int V, int H, int W, float voxel_size, const float* origin_host,
                             const int32_t* coords, int n, uint8_t* cnt, void* stream);
int o2345_costvol_gather_list(const float* feats_nhwc, const float* proj, int V, int H, int W, int C, float voxel_size,
                              const float* origin_host, const uint8_t* cnt_row, const int32_t* coords, int n_rows,
                              float* out_rows, void* stream);
int o2345_build_index_grid(const int32_t* coords, int n, int ts, int nx, int ny, int nz, int32_t* grid, void* stream);
/* replaces the prune() of get_valid_sparse_coords_by_sdf (sparse_neus_renderer.py:838-848): out[v] = mask[v] > 0 and any
 * |sdf| < threshold within the (2*radius+1)^3 box around v (the reference's avg_pool3d(7) > 0 dilation: radius 3). */
int o2345_prune_dilate(const float* sdf, const float* mask, int D, float threshold, int radius, uint8_t* out, void* stream);
/* replaces: tsparse/torchsparse_utils.py:125 sparse_to_dense_channel + sparse_sdf_network.py:252 sparse_to_dense_volume.
 * rows [N,C] -> dense_cl [D^3,C] (channel-last, what the samplers here read), dense_cf [C,D^3] (the reference's
 * [1,C,X,Y,Z]) and mask [D^3]; any output may be NULL. */
int o2345_scatter_dense(const float* rows, const int32_t* row_of_voxel, int C, long long nvox, float* dense_cl,
                        float* dense_cf, float* mask, void* stream);

/* ---- sparse cost-regularisation CNN (replaces torchsparse v1.4.0: SparseTensor kernel maps, spnn.Conv3d,
 * spnn.BatchNorm, spnn.ReLU as used by tsparse/modules.py:94-124,259-304) -------------------------------------------- */
size_t o2345_sparse_downsample_workspace_bytes(int nxc, int nyc, int nzc);
/* spdownsample(stride 2, kernel 3): coarse level (cell size 2*ts) from the fine coordinates. */
int o2345_sparse_downsample(const int32_t* coords_fine, int n_fine, int ts, int nxc, int nyc, int nzc,
                            int32_t* row_of_cell, int32_t* coords_coarse, int32_t* n_coarse_dev, void* workspace,
                            size_t workspace_bytes, void* stream);
/* spnn.Conv3d(kernel 3, no bias).  mode 0: stride 1; 1: stride 2 (in = finer level); 2: transposed stride 2
 * (in = coarser level).  in_grid: the index grid (gx,gy,gz cells) of the INPUT level; kernel [27,cin,cout]. */
int o2345_sparse_conv3d(int mode, const float* in, int cin, const int32_t* in_grid, int gx, int gy, int gz,
                        const int32_t* out_coords, int n_out, int ts_out, const float* kernel, int cout, float* out,
                        void* stream);
/* the same convolution on the f16 matrix cores in split precision (fp32-class accuracy, see o2345_sdf_mlp_x3);
 * wblob: the kernel packed by weights.pack_sparse_conv_x3, o2345_sparse_conv_x3_blob_floats(cin, cout) floats.
 * identity_rows != 0 (mode 0 only): the CALLER GUARANTEES that out_coords is the coordinate list in_grid was built from, in the same order
 * (output row q = input row q, n_out = number of input rows) -- what a stride-1 spnn.Conv3d always produces.  Only then may the LDS-tiled brick
 * kernel run (32 -> 16 channels: it writes out[in_grid[site]] and never reads out_coords); with identity_rows = 0 every shape takes the gather
 * form, which honours any subset / order of out_coords. */
int o2345_sparse_conv_x3_blob_floats(int cin, int cout);
int o2345_sparse_conv3d_x3(int mode, const float* in, int cin, const int32_t* in_grid, int gx, int gy, int gz,
                           const int32_t* out_coords, int n_out, int ts_out, const float* wblob, int cout, int identity_rows, float* out,
                           void* stream);
size_t o2345_bn_workspace_bytes(int C);
/* spnn.BatchNorm in training mode (batch statistics; the reference never calls .eval()) + activation (+ skip):
 * y = act(bn(x)) [+ skip]; slope 0 = ReLU.  mean_var_out [2,C] optional. */
int o2345_bn_act_rows(const float* x, int n, int C, const float* gamma, const float* beta, float eps, float slope,
                      int abs_gamma, const float* skip, float* y, float* mean_var_out, void* workspace,
                      size_t workspace_bytes, void* stream);
/* replaces inplace_abn.InPlaceABN forward (featurenet.py:12-22, sparse_sdf_network.py:171-173): batch-stat BN +
 * leaky ReLU on [V,C,H,W], C in {8, 16, 32}; writes NCHW and/or channel-last NHWC. */
size_t o2345_abn_workspace_bytes(int C);
int o2345_abn_nchw(const float* x, int V, int C, int H, int W, const float* gamma, const float* beta, float eps,
                   float slope, int abs_gamma, float* y_nchw, float* y_nhwc, void* workspace, size_t workspace_bytes,
                   void* stream);

/* ---- SDF network (replaces ops/grid_sampler.py:64 grid_sample_3d + models/embedder.py:63 Embedding +
 * sparse_sdf_network.py:35 LatentSDFLayer, :402 sdf(), :476 gradient(), and the per-chunk loop of
 * sparse_neus_renderer.py:881 extract_fields) ------------------------------------------------------------------------
 * blob: o2345_sdf_blob_floats() floats packed by weights.pack_sdf_blob.  vol_cl: [D,D,D,16] channel-last.
 * variant 0: SDF only; 1: all 128 outputs; 2: SDF + d sdf/d x.  Points: pts [P,3], or pts = NULL and grid_R = R for
 * the x-major lattice linspace(-1,1,R)^3.  index / n_dev: optional list of point slots and device-side count.
 * out_sdf[slot] = sign * sdf. */
int o2345_sdf_blob_floats(void);
int o2345_sdf_mlp(int variant, const float* blob, const float* vol_cl, int D, const float* pts, const int32_t* index,
                  const int32_t* n_dev, long long n, int grid_R, float sign, float* out_sdf, float* out_feat,
                  float* out_lat, float* out_grad, void* stream);
/* same, with lat_in [P,16]: use the given latent per point instead of sampling the volume (replaces
 * sparse_sdf_network.py:441 get_sdf_volume: SDF at voxel centres with the voxel's own latent); variants 0/1, explicit points. */
int o2345_sdf_mlp_ex(int variant, const float* blob, const float* vol_cl, int D, const float* pts, const int32_t* index,
                     const int32_t* n_dev, long long n, int grid_R, float sign, const float* lat_in, float* out_sdf,
                     float* out_feat, float* out_lat, float* out_grad, void* stream);
/* fp32-class accuracy on the f16 matrix cores: every operand split into two f16 halves (hi + lo, 22 bits) and each product
 * accumulated in fp32 as hi*hi + hi*lo + lo*hi -- three v_mfma_f32_32x32x16_f16 instead of eight fp32 MFMAs per 16 k.
 * Same function as o2345_sdf_mlp variant 0 within ~1e-6 (tests/test_gpu_parity.py::test_sdf_mlp_x3). */
int o2345_sdf_mlp_x3(const float* blob, const float* vol_cl, int D, const float* pts, const int32_t* index, const int32_t* n_dev,
                     long long n, int grid_R, float sign, float* out_sdf, void* stream);
/* SDF + analytic gradient, wide layers (144->128 and its transpose) split-f16, the 40-wide layer 0 on the exact fp32 MFMA */
int o2345_sdf_grad_x3(const float* blob, const float* vol_cl, int D, const float* pts, const int32_t* index, const int32_t* n_dev,
                      long long n, int grid_R, float sign, float* out_sdf, float* out_grad, void* stream);
/* extract_fields on the lattice with layer 0 of the SDF network TABULATED (ABI 1.3): on the x-major lattice linspace(-1,1,R)^3 the first layer's
 * pre-activation is separable, b0 + W0 . PE(x,y,z) = Txy[ix,iy] + Tz[iz].  tab_axes [3][R][128]: per-axis tables in the kernels' lane order
 * (weights.sdf_grid_tables); sdf_grid_tables adds x + y + bias into tab_xy [R*R][128]; sdf_grid_x3 evaluates out_sdf [R^3] = sign * sdf with
 * tab_xy and tab_z = tab_axes + 2*R*128.  Same network as o2345_sdf_mlp_x3 with pts = NULL, grid_R = R, minus 18 sincos and 36 matrix steps per tile. */
int o2345_sdf_grid_tables(const float* tab_axes, const float* bias_lane_order, int grid_R, float* tab_xy, void* stream);
int o2345_sdf_grid_x3(const float* blob, const float* vol_cl, int D, int grid_R, float sign, const float* tab_xy, const float* tab_z,
                      float* out_sdf, void* stream);
/* o2345_sdf_grid_x3 evaluated only where the scene has a latent (additive since 2.1).  maskvol [D^3]: the occupancy volume (0 = unkept).
 * The CALLER GUARANTEES (a) that vol_cl is zero wherever maskvol is zero -- what o2345_scatter_dense writes -- and (b) that background [R^3] is
 * o2345_sdf_grid_x3's out_sdf for the same blob, tab_xy and tab_z with sign = +1 on a latent volume of zeros (any D: a 2^3 one will do).
 * A lattice point whose trilinear sampler is off (index 0 of an axis) or none of whose eight corner voxels is kept samples a latent of exactly
 * zero, so its SDF is the background's: a pre-pass copies sign * background into every aligned tile of 32 slots without an active point and lists
 * the slots of the other tiles (device-side count, no read-back); only those run the network.  out_sdf equals o2345_sdf_grid_x3's bit for bit.
 * With a volume that breaks (a), the points whose corners are all unkept get the background's value instead of the volume's.
 * workspace: o2345_sdf_grid_sparse_workspace_bytes(grid_R) bytes, 16-byte aligned (0 = grid_R out of range: needs 2 <= grid_R, grid_R^3 < 2^31). */
size_t o2345_sdf_grid_sparse_workspace_bytes(int grid_R);
int o2345_sdf_grid_sparse_x3(const float* blob, const float* vol_cl, const float* maskvol, int D, int grid_R, float sign, const float* tab_xy,
                             const float* tab_z, const float* background, float* out_sdf, void* workspace, size_t workspace_bytes, void* stream);

/* ---- ray rendering (replaces models/sparse_neus_renderer.py:457 render and everything it calls) ------------------
 * Per-sample arrays are sample-major [S][R]. */
int o2345_ray_coarse(const float* rays_o, const float* rays_d, int R, float near, float far, int S, float* z, float* pts,
                     void* stream);
/* the same with the reference's stratified jitter (models/sparse_neus_renderer.py:506-515): t_rand [R][S] (ray-major, what
 * torch.rand(z_vals.shape) returns) or NULL */
int o2345_ray_coarse_jitter(const float* rays_o, const float* rays_d, int R, float near, float far, int S,
                            const float* t_rand, float* z, float* pts, void* stream);
/* the same with per-ray near / far [R] (the reference broadcasts near + (far - near) * linspace per ray, :486-490) */
int o2345_ray_coarse_per_ray(const float* rays_o, const float* rays_d, int R, const float* near_ray, const float* far_ray, int S,
                             const float* t_rand, float* z, float* pts, void* stream);
/* up_sample + sample_pdf of one round (:73-115, render_utils.py:8-51): z / sdf [S][R] sorted per ray -> new_z [n_imp][R], their points, new_sdf = 100
 * (the cat_z_vals default), and the list of new points inside the mask (slots t * R + r) with its device-side count.  wbuf: scratch [S][R] floats for
 * the streaming kernel, or NULL: the LDS-staged kernel then runs whatever R is (the two give bit-identical results; csrc/render.hip). */
int o2345_ray_upsample(const float* rays_o, const float* rays_d, int R, const float* z, const float* sdf, int S,
                       float inv_s, const float* maskvol, int D, float* wbuf, int n_imp, float* new_z, float* new_pts,
                       float* new_sdf, int32_t* list, int32_t* count_dev, void* stream);
int o2345_ray_merge(int R, float* z, float* sdf, int S, float* new_z, float* new_sdf, int n_new, void* stream);
/* finalize: mid points, section lengths, occupancy of the mid points and the list of occupied slots; every slot of sdf / grad / rgb receives the
 * reference's defaults (sdf = 100, grad = rgb = 0; models/sparse_neus_renderer.py:231), occupied or not -- a caller may evaluate any part of the list.
 * (o2345_render_rays, which evaluates every list entry, uses an internal variant that skips the occupied slots.) */
int o2345_ray_finalize(const float* rays_o, const float* rays_d, int R, const float* z, int S, float sample_dist,
                       const float* maskvol, int D, float* mid_z, float* dists, float* pts, float* pm, float* sdf,
                       float* grad, float* rgb, int32_t* list, int32_t* count_dev, void* stream);
int o2345_ray_composite(const float* rays_o, const float* rays_d, int R, int S, const float* mid_z, const float* dists,
                        const float* pm, const float* sdf, const float* grad, const float* rgb, const uint8_t* nviews,
                        float inv_s, float alpha_inter_ratio, float background, float* color, float* depth,
                        float* weights, float* cdf, float* weights_sum, float* weights_max, float* depth_var,
                        float* alpha_sum, float* grad_err, uint8_t* color_mask, void* stream);

/* One render() call (models/sparse_neus_renderer.py:457-635).  The struct is declared HERE only: csrc/ includes this header, the ctypes binding
 * generates its Structure from this text and checks it against o2345_struct_size / o2345_struct_layout of the loaded library. */
typedef struct O2345RenderIO {
    /* scene */
    const float* sdf_blob;          /* weights.pack_sdf_blob */
    const float* color_x3_blob;     /* split-f16 colour network (weights.pack_color_x3_blob); takes precedence */
    const float* color_mfma_blob;   /* fp32 matrix-core colour network (weights.pack_color_mfma_blob); one of the two is required */
    const float* vol_cl;            /* [D,D,D,16] */
    const float* maskvol;           /* [D^3] */
    const float* cmaps;             /* [V,H,W,64] */
    const float* proj;              /* [V,3,4] */
    const float* cam_pos;           /* [V,3] */
    int D, V, H, W;
    /* rays */
    const float* rays_o; const float* rays_d;
    const float* near_ray;          /* optional [R]: per-ray near / far (the reference's [N_rays,1] form, :486-490); NULL: the scalars below */
    const float* far_ray;
    const float* query_cam;         /* [3] */
    const float* t_rand;            /* optional [R][n_samples]: the reference's perturb > 0 jitter, drawn by the caller */
    int R, n_samples, n_importance;
    int sdf_mode;                   /* 0: exact fp32 MFMA SDF kernels; 2: split-f16 ("f16x3", fp32-class accuracy).  (ABI 1.x called this sdf_bf16.) */
    int segment_rays;               /* 0: the call is ONE render() call of the reference.  > 0 (a multiple of 64): the R rays are consecutive render() calls of
                                     * segment_rays rays each (the last one may be shorter) evaluated together -- the reference's two per-call rules (cat_z_vals' "more
                                     * than one new point inside the mask", :137; render_core's "first 100 points when nothing is occupied", :222-223) are applied
                                     * PER SEGMENT, t_rand holds the segments' draws back to back, and `scalars` becomes [ceil(R / segment_rays)][4] */
    float near, far;                /* used when near_ray == NULL */
    float sample_dist;              /* length of the last section (:484: ((far - near) / n_samples).mean()); <= 0: (far - near) / n_samples */
    float inv_s, alpha_inter_ratio, background;
    float weight_cull;              /* 0: the colour network is evaluated on every occupied sample, like the reference.  > 0: only on occupied samples whose
                                     * compositing weight w = alpha * T (the value `weights` returns, computed first from the SDF / gradient pass) is >= weight_cull;
                                     * the others keep rgb = 0.  Every colour component lies in [0, 1] (a softmax blend of source pixels), so a ray's colour moves
                                     * by at most S * weight_cull: 128 * 2^-24 = 7.6e-6 at the default 2^-24, below the 3e-5 stage tolerance.  depth, weights,
                                     * gradients and the colour mask (valid-view counts of culled points come from the counting kernel) are unaffected.  Only samples
                                     * BEHIND a surface qualify: in free space the reference's +1e-5 in alpha keeps w ~ 1e-5 (:349-375), those are never dropped. */
    /* outputs: per-sample arrays are sample-major [S][R] (+[,3]) */
    float* mid_z; float* dists; float* pm; float* sdf; float* grad; float* rgb; uint8_t* nviews;
    float* color; float* depth; float* weights; float* cdf; float* weights_sum; float* weights_max; float* depth_var;
    float* alpha_sum; float* grad_err; uint8_t* color_mask;
    float* z_vals;                  /* optional [S][R] */
    float* scalars;                 /* optional [4]: alpha_sum.mean(), alpha_sum.sum() / (R S), sum grad_err[.,0] / (sum grad_err[.,1] + 1e-5), number of
                                     * evaluated list entries (fixed-order fp64 reduction, deterministic): the scalar entries of render()'s returned
                                     * dict (alpha_sum, alpha_mean, gradient_error_fine; :586-633) without a pass over the per-ray arrays */
    unsigned long long* color_stats;/* optional [4] device counters the colour kernel ADDS to (diagnostics, caller-owned and caller-zeroed): (32-point tile,
                                     * view) pairs evaluated in the pooling pass / the network pass, tiles, tiles that evaluated every view */
} O2345RenderIO;
/* The occupied-point list of a render call grouped, stably, by view-visibility signature (bit v = the point projects inside view v): every 32-point tile of the
 * colour kernels then holds points that see the same views, and the kernels skip the views nobody sees.  The network kernels scatter by slot, so their
 * results do not depend on the order (no reference counterpart: the reference evaluates every (point, view) pair, models/projector.py:96-228).
 * list [<= n_max] slots, *count_dev entries (device-side count); list_out != list; keys_out (optional) receives the signatures in output order. */
size_t o2345_list_sort_workspace_bytes(long long n_max, int V);
int o2345_list_sort_by_visibility(const float* pts, const int32_t* list, const int32_t* count_dev, long long n_max, const float* proj, int V, int H, int W,
                                  int32_t* list_out, uint32_t* keys_out, void* workspace, size_t workspace_bytes, void* stream);
/* V: the scene's view count -- the list-sort buffers are part of the workspace only when the call will sort its list (V <= 32 and at least 2^20 sample slots) */
size_t o2345_render_workspace_bytes(int R, int n_samples, int n_importance, int V);
int o2345_render_rays(const O2345RenderIO* io_host, void* workspace, size_t workspace_bytes, void* stream);

/* proj [V,3,4] = intrinsics [V,3,3] @ w2cs[:, :3, :] (models/render_utils.py:106) and cam_pos [V,3] = inverse(w2cs)[:, :3, 3] (models/projector.py:60-70)
 * in ONE launch, no BLAS / solver library behind it (the first torch.matmul + torch.inverse of a process cost 180 ms of library initialisation
 * inside the reference's own timing bracket).  Products are fp32 FMA chains in k order (what rocBLAS / ATen evaluate for k = 3); the inverse is a
 * general 4x4 inverse by cofactors in fp64, rounded once to fp32 (singular w2c: cam_pos = inf / nan like torch.inverse's). */
int o2345_camera_terms(const float* intrinsics, const float* w2cs, int V, float* proj_out, float* cam_pos_out, void* stream);

/* ---- colour blending (replaces models/projector.py:96 Projector.compute / :231 compute_view_independent +
 * models/rendering_network.py:75 GeneralRenderingNetwork.forward) ---------------------------------------------------
 * cmaps [V,H,W,64] = rgb(3) | features(56) | pad; proj [V,3,4] = K @ w2c[:3]; cam_pos [V,3].
 * H and W are independent (each > 1; the reference's img_wh = [W, H]).  A view sees a point if |gx| < 1 and |gy| < 1 -- the border of the image does
 * NOT count here (models/projector.py:188-190), unlike in the cost volume -- and the point is geometrically valid; every entry below that reports a
 * number of views (o2345_view_count*, out_nviews of the colour entries, the mask of o2345_project_features) reports the same number for the same
 * point, also within rounding of a border: o2345_view_count* divides, the colour kernels multiply by a reciprocal and correct the quotient once, and
 * tests/test_gpu_project_units.py holds the two to equal counts on points aimed at the borders.  The signature of o2345_list_sort_by_visibility above
 * is the same strict test written without a division; it may differ from the mask within rounding of a border, which only affects how points are
 * grouped. */
int o2345_pack_color_maps(const float* feat_nchw, const float* color_nchw, int V, int H, int W, float* out_nhwc64,
                          void* stream);
int o2345_view_count(const float* pts, long long n, const float* maskvol, int D, const float* proj, int V, int H, int W,
                     uint8_t* out, void* stream);
/* the same count only where skip_if_positive[i] <= 0 (NULL: everywhere): the colour kernels write out_nviews for the points they evaluate */
int o2345_view_count_unlisted(const float* pts, long long n, const float* skip_if_positive, const float* maskvol, int D, const float* proj,
                              int V, int H, int W, uint8_t* out, void* stream);
/* Projector + GeneralRenderingNetwork fused, every linear layer on fp32 MFMA (k_color_pts, csrc/color_pts.hip: a wave owns 32 points and walks the
 * views; any V in [1,255]); blob from weights.pack_color_mfma_blob.  pts [P,3]; index / n_dev: optional list of point slots + device-side count;
 * exactly one of query_cam [3] (Projector.compute) / normals [P,3] (compute_view_independent).  out_rgb [P,3], out_nviews [P] (optional).
 * View counts, three regimes (tests/test_gpu_many_views.py runs each): counts of valid views are uint8, so every entry that takes V
 * (o2345_color_points_*, o2345_color_from_features, o2345_project_features, o2345_view_count*, o2345_costvol_index) accepts 1 .. 255 and refuses 0 and
 * 256 with an error status before it writes anything; the wave-uniform skip of the views that see none of a tile's 32 points keeps a 64-bit mask of
 * active views and exists for V <= 64 -- from 65 views on every (tile, view) pair is evaluated, same results; o2345_list_sort_by_visibility has a
 * 32-bit signature and refuses V > 32, and o2345_render_rays groups its point list with it only for V <= 32 (above, the list stays in emission
 * order and o2345_render_workspace_bytes lays the workspace out without the sort's buffers).
 * stats_dev (optional, [4], caller-owned and caller-zeroed): work counters the launch ADDS to -- (32-point tile, view) pairs evaluated in the
 * pooling pass / the network pass, tiles, tiles that evaluated every view.  (ABI 1.x kept these in a process-global buffer; the pure-VALU
 * kernel o2345_color_points of ABI 1.x is gone: 206 ms against 37.) */
int o2345_color_mfma_blob_floats(void);
int o2345_color_points_mfma(const float* blob, const float* vol_cl, const float* maskvol, int D, const float* cmaps,
                            const float* proj, const float* cam_pos, int V, int H, int W, const float* pts,
                            const int32_t* index, const int32_t* n_dev, long long n, const float* query_cam,
                            const float* normals, float* out_rgb, uint8_t* out_nviews, unsigned long long* stats_dev, void* stream);
/* same kernel, split-f16 matrix steps (hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16, fp32 accumulate; fp32-class
 * accuracy, see o2345_sdf_mlp_x3); blob from weights.pack_color_x3_blob */
int o2345_color_x3_blob_floats(void);
int o2345_color_points_x3(const float* blob, const float* vol_cl, const float* maskvol, int D, const float* cmaps,
                          const float* proj, const float* cam_pos, int V, int H, int W, const float* pts,
                          const int32_t* index, const int32_t* n_dev, long long n, const float* query_cam,
                          const float* normals, float* out_rgb, uint8_t* out_nviews, unsigned long long* stats_dev, void* stream);
/* the two entries above with a tile queue: the 32-point tiles are not dealt to the waves in advance but claimed by whichever wave is free.
 * tile_queue: 8 ints of caller device memory, cleared by the call on `stream` and in use until the launch has finished (one per launch in flight).
 * Outputs and the sums in stats_dev are bit-identical to theirs. */
int o2345_color_points_mfma_q(const float* blob, const float* vol_cl, const float* maskvol, int D, const float* cmaps,
                              const float* proj, const float* cam_pos, int V, int H, int W, const float* pts,
                              const int32_t* index, const int32_t* n_dev, long long n, const float* query_cam,
                              const float* normals, float* out_rgb, uint8_t* out_nviews, unsigned long long* stats_dev, int32_t* tile_queue, void* stream);
int o2345_color_points_x3_q(const float* blob, const float* vol_cl, const float* maskvol, int D, const float* cmaps,
                            const float* proj, const float* cam_pos, int V, int H, int W, const float* pts,
                            const int32_t* index, const int32_t* n_dev, long long n, const float* query_cam,
                            const float* normals, float* out_rgb, uint8_t* out_nviews, unsigned long long* stats_dev, int32_t* tile_queue, void* stream);
/* GeneralRenderingNetwork.forward on MATERIALISED inputs in the reference's own (view-major) layout (models/rendering_network.py:75-129):
 * geometry_feat [P,16], rgb_feat [V,P,59] (colours | features), ray_diff [V,P,4], mask [V,P] (non-zero = valid) -> rgb [P,3] and the number of
 * valid views [P] (optional).  blob: the x3 (x3 = 1) or fp32-MFMA (x3 = 0) packing of the network.  The fused Projector path above is the fast
 * one; this entry makes the network a drop-in on its own (any Projector). */
/* Projector.compute (query_cam) / compute_view_independent (normals) MATERIALISED (models/projector.py:96-425): the four tensors of
 * GeneralRenderingNetwork.forward in the reference's layout -- geometry_feat [P,16], rgb_feat [V,P,59], ray_diff [V,P,4], mask [V,P] (1 / 0).
 * For callers that want the tensors themselves (a foreign rendering network); the fused o2345_color_points_* never store them. */
int o2345_project_features(const float* vol_cl, const float* maskvol, int D, const float* cmaps, const float* proj, const float* cam_pos, int V,
                           int H, int W, const float* pts, long long P, const float* query_cam, const float* normals, float* geometry_feat,
                           float* rgb_feat, float* ray_diff, float* mask, void* stream);
int o2345_color_from_features(const float* blob, int x3, const float* geometry_feat, const float* rgb_feat, const float* ray_diff,
                              const float* mask, int V, long long P, float* out_rgb, uint8_t* out_nviews, void* stream);

/* ---- marching cubes (replaces mcubes.marching_cubes, call site models/sparse_neus_renderer.py:932) -----------------
 * u [n0,n1,n2] float32 on the device; iso is a DOUBLE like PyMCubes' isovalue (ABI 1.2).  count() synchronises the stream and returns the sizes on the host;
 * emit() writes verts float64 [nv,3] (index coordinates) and tris int32/int64 [nt,3]. */
size_t o2345_mc_workspace_bytes(int n0, int n1, int n2);
int o2345_marching_cubes_count(const float* u, int n0, int n1, int n2, double iso, void* workspace,
                               size_t workspace_bytes, long long* nv_host, long long* nt_host, void* stream);
int o2345_marching_cubes_emit(const float* u, int n0, int n1, int n2, double iso, void* workspace, double* verts,
                              void* tris, int index_bytes, void* stream);

/* ---- mesh components (additive since 2.1: drops the detached blobs of an extracted mesh before it is coloured and written; the reference has no such step,
 * its users run mesh.split() afterwards) -------------------------------------------------------------------------------------------------
 * Component: vertices connected through triangles that share vertex INDICES; a vertex no triangle references is a component with 0 faces.  Label of a
 * vertex: the smallest vertex index of its component.  Size: its number of faces.  Selection: min_faces = n keeps components with >= n faces;
 * keep_largest keeps only the one with the most faces (ties: smaller label), among what min_faces left; with any selection active 0-face components
 * are dropped; with none (min_faces <= 0, keep_largest = 0) everything is kept.  A triangle is kept iff its first vertex is.  Exact and deterministic.
 * tris device int32 / int64 [nt,3] (index_bytes 4 / 8); nv, nt >= 0, nv * 3 < 2^31.  workspace: mesh_components_workspace_bytes(nv, nt) bytes, 16-byte aligned.
 * count() (synchronises the stream once) returns on the HOST the number of components, of kept components, of kept vertices and triangles, and writes
 * the labels (device int32 [nv]) when `labels` is not NULL; a triangle index outside [0, nv) is an error.  emit() (same workspace, untouched in between):
 * verts device fp64 [nv,3] -> verts_out [nv_kept,3] bit for bit and in order, tris_out [nt_kept,3] (same index width) renumbered by the exclusive scan of
 * the vertex keep flags, kept_out device int32 [nv_kept] = new -> old vertex index.  Any output may be NULL. */
size_t o2345_mesh_components_workspace_bytes(long long nv, long long nt);
int o2345_mesh_components_count(const void* tris, int index_bytes, long long nv, long long nt, long long min_faces, int keep_largest, void* workspace,
                                size_t workspace_bytes, int* labels, long long* n_components_host, long long* n_components_kept_host,
                                long long* nv_kept_host, long long* nt_kept_host, void* stream);
int o2345_mesh_components_emit(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, void* workspace, double* verts_out,
                               void* tris_out, int* kept_out, void* stream);

/* ---- vertex adjacency and Taubin smoothing (additive since 2.1; the reference has no such step, its users smooth the mesh in another tool) ----------
 * Adjacency: every triangle (a, b, c) contributes the ordered pairs (a,b), (b,a), (b,c), (c,b), (c,a), (a,c), minus those with equal ends.  Row v of the
 * CSR table holds the distinct second elements of the pairs that start at v, ascending; the multiplicity of u in row v (the number of such pairs) is the
 * number of triangles on edge {u, v}; boundary[v] = 1 iff some entry of row v has multiplicity exactly 1.  An unreferenced vertex has an empty row and
 * boundary 0.  Independent of face order and of the rotation of a triangle's indices.  Exact and deterministic.
 * tris device int32 / int64 [nt,3] (index_bytes 4 / 8); 0 <= nv < 2^30, 6 * nt < 2^31.  workspace: mesh_adjacency_workspace_bytes(nv, nt) bytes, 16-byte
 * aligned.  count() builds the whole table inside the workspace and returns its number of entries on the HOST (synchronises the stream once); a triangle
 * index outside [0, nv) is an error.  emit() (same workspace and nv, untouched in between) writes offsets device int32 [nv + 1], neighbours device int32
 * [n_entries] (may be NULL when that is 0) and boundary device uint8 [nv].
 * Smoothing: one step with factor f computes every vertex from the OLD positions in fp64: acc = 0; acc = acc + p[u] over the neighbours u in ascending
 * order, per coordinate; m = acc / deg; d = m - p[v]; p'[v] = p[v] + f * d with separate multiply and add.  A vertex with deg = 0, or with boundary[v] = 1
 * when `boundary_or_null` is given, keeps its value bit for bit.  mesh_smooth runs `iterations` times step(lam), then step(mu) unless mu == 0
 * (0 < lam <= 1, mu <= 0, both finite: Taubin's filter; mu = 0 is plain Laplacian smoothing).  verts_in device fp64 [nv,3] is only read; the result is in
 * verts_out [nv,3] for every iteration count (0: a copy); verts_tmp [nv,3] is scratch (may be NULL when at most one step runs).  The three must differ. */
size_t o2345_mesh_adjacency_workspace_bytes(long long nv, long long nt);
int o2345_mesh_adjacency_count(const void* tris, int index_bytes, long long nv, long long nt, void* workspace, size_t workspace_bytes,
                               long long* n_entries_host, void* stream);
int o2345_mesh_adjacency_emit(void* workspace, long long nv, int* offsets, int* neighbours, unsigned char* boundary, void* stream);
int o2345_mesh_smooth(const double* verts_in, long long nv, const int* offsets, const int* neighbours, const unsigned char* boundary_or_null, int iterations,
                      double lam, double mu, double* verts_tmp, double* verts_out, void* stream);

/* ---- decimation by vertex clustering (additive since 2.1; the reference has no such step, its users simplify the mesh in another tool) ---------------
 * q = floor(p / cell) per axis in fp64 (IEEE division); the vertices with equal q form a cluster, whose representative is its smallest member index.
 * Per axis max q - min q must be below 2^21 (the three offsets pack into one 63-bit key; negative coordinates are legal).  Triangle (a, b, c) maps to
 * its corners' clusters; it is degenerate, and dropped, iff two mapped corners are equal; of the others, those over the same SET of three clusters are
 * duplicates whatever their orientation or rotation, and the first in face order is kept.  Kept triangles keep face order, corner order and
 * orientation.  A cluster is kept iff a kept triangle references it; kept clusters are numbered by an exclusive scan of "is a kept representative" over
 * the old vertex order.  Position of a kept cluster, per coordinate: acc = 0; acc = acc + p[u] over its members u in ascending index order, one
 * sequential sum; acc / count.  Exact and deterministic: equal to mesh_io.decimate_mesh to the last bit.  No manifoldness is promised: where a thin part
 * collapses, clustering leaves edges with more than two triangles, or open ones.
 * verts device fp64 [nv,3], tris device int32 / int64 [nt,3] (index_bytes 4 / 8), both only read; 0 <= nv < 2^30, 3 * nt < 2^31; cell finite and > 0.
 * workspace: mesh_decimate_workspace_bytes(nv, nt) bytes (0 for bad sizes), 16-byte aligned.  count() does all the work inside the workspace and
 * returns on the HOST (synchronises the stream once) the number of clusters, of output vertices and triangles, and of degenerate and duplicate
 * triangles dropped.  Errors: a bad cell, bad sizes, a workspace that is too small, a non-finite coordinate, a triangle index outside [0, nv), an
 * extent of 2^21 cells or more; the last three are counted on the device, never dereferenced.  emit() (same workspace, nv and nt, untouched in between)
 * writes verts_out device fp64 [nv_out,3], tris_out [nt_out,3] of the input's width and cluster device int32 [nv] (the new index of every old vertex's
 * cluster, or -1); any of the three may be NULL. */
size_t o2345_mesh_decimate_workspace_bytes(long long nv, long long nt);
int o2345_mesh_decimate_count(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, double cell, void* workspace,
                              size_t workspace_bytes, long long* n_clusters_host, long long* nv_out_host, long long* nt_out_host,
                              long long* n_degenerate_host, long long* n_duplicate_host, void* stream);
int o2345_mesh_decimate_emit(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, void* workspace, double* verts_out,
                             void* tris_out, int* cluster, void* stream);

/* ---- projection of the vertices onto a level set of the SDF (additive since 2.1; the reference has no such step: its marching-cubes vertices,
 * sparse_neus_renderer.py:907-937, lie on the zero set only as far as linear interpolation along a grid edge allows, and validate_colored_mesh,
 * trainer_generic.py:1309-1363, colours them where they are) ------------------------------------------------------------------------------------------
 * A few Newton steps p <- p - (s - level) g / |g|^2 per vertex, (s, g) from the SDF kernels of this library (sdf_mode 0: o2345_sdf_mlp_ex variant 2;
 * 2: o2345_sdf_grad_x3; sign 1).  Index units (one grid spacing = 1); bmin / bmax = the float32 bounds widened to fp64, ext = bmax - bmin; all of the
 * following in fp64, one operation at a time, in the order written, without a square root.  World point w_k = x_k / (R - 1) * ext_k + bmin_k; the network
 * sees float32(w).  A round evaluates (s, g) at every ACTIVE vertex (all in round 0); then, o the input position and x the current one:
 *   r = |double(s) - level|;  s or g non-finite, or g2 = (gx gx + gy gy) + gz gz not > 0: STALLED, the vertex leaves the active set and keeps x;
 *   else r <= tol: CONVERGED, leaves and keeps x;  else, in rounds 0 .. iterations - 1: t = (double(s) - level) / g2, d_k = t g_k,
 *   e_k = d_k / ext_k * (R - 1) clamped to [-max_step, max_step] per axis, y_k = x_k - e_k clamped to [o_k - max_move, o_k + max_move], then to
 *   [0, R - 1], x <- y; each of the three clamps that changes a value counts one clamped event;  else (round `iterations` only classifies): UNCONVERGED.
 * Exact and deterministic: equal to mesh_io.project_vertices, given these kernels as its field, to the last bit; the order of the active lists
 * changes between runs and does not change a result.  Not promised: that a vertex stays on its sheet of the surface beyond the max_move box, or that
 * triangles keep their orientation where the surface folds inside one cell.
 * blob, vol_cl, D as for o2345_sdf_mlp; verts device fp64 [nv,3], only read; 0 <= nv < 2^30; grid_R >= 2; bound_min / bound_max HOST float32 [3] as
 * for o2345_mesh_pack_vertices, bound_max > bound_min; iterations in [1, 64]; level finite; tol finite, >= 0; max_step, max_move finite, > 0.
 * workspace: mesh_project_workspace_bytes(nv) bytes (0 for bad sizes), 16-byte aligned.  verts_out device fp64 [nv,3], not verts.  stats: device,
 * 8-byte aligned, written by this call.  No host synchronisation: all rounds are queued at once, the counts stay on the device.  A non-zero
 * n_nonfinite means bad input: the caller raises (the affected vertices stall, nothing is dereferenced through them).  Errors: bad arguments, a
 * workspace that is too small. */
typedef struct O2345ProjectStats {
    unsigned long long n_nonfinite;                     /* vertices with a non-finite coordinate */
    unsigned long long converged, unconverged, stalled;
    unsigned long long clamped;                         /* clamped events */
    unsigned long long max_before, max_after;           /* the bit pattern of a non-negative double: the max of r in round 0; the max of the r at which the
                                                         * vertices left or ended; non-finite r take no part; 0 for an empty mesh */
    unsigned long long reserved;                        /* 0 */
    int count[66];                                      /* active vertices per round, entries 0 .. iterations; the rest 0 */
} O2345ProjectStats;
size_t o2345_mesh_project_workspace_bytes(long long nv);
int o2345_mesh_project(const float* blob, const float* vol_cl, int D, int sdf_mode, const double* verts, long long nv, int grid_R, const float* bound_min_host,
                       const float* bound_max_host, int iterations, double level, double tol, double max_step, double max_move, void* workspace,
                       size_t workspace_bytes, double* verts_out, O2345ProjectStats* stats, void* stream);

/* ---- mesh serialisation (replaces the numpy / trimesh tail of validate_mesh and validate_colored_mesh,
 * models/trainer_generic.py:1287-1303, 1365-1382: index -> world frame, scale_mat, trans_mat, uint8 colours, PLY records) -----
 * verts_idx: device fp64 [n,3] index coordinates on an R^3 grid (o2345_marching_cubes_emit); bound_min/max [3], scale_mat and
 * trans_mat (4x4 row-major fp32, may be NULL) are HOST arrays; rgb device fp32 [n,3] or NULL.
 * vertex_records: n x (3 x float32 [+ rgba uint8]) = 16 (12 without colours) bytes each; face_records: m x (uint8 3, 3 x int32). */
int o2345_mesh_pack_vertices(const double* verts_idx, long long n, int grid_R, const float* bound_min_host, const float* bound_max_host,
                             const float* scale_mat_host, const float* trans_mat_host, const float* rgb, uint8_t* vertex_records, void* stream);
int o2345_mesh_pack_faces(const void* tris, int index_bytes, long long m, uint8_t* face_records, void* stream);
/* extract_geometry's index -> world step on the device, in place and in fp64 (sparse_neus_renderer.py:936: vertices / (R - 1) * (bound_max - bound_min)
 * + bound_min; the same IEEE expression numpy evaluates): verts [n,3] device fp64; extent = bound_max - bound_min (the reference subtracts the fp32 bounds,
 * THEN promotes) and offset = bound_min as HOST fp64 [3]. */
int o2345_mc_verts_to_world(double* verts, long long n, int grid_R, const double* extent_host, const double* offset_host, void* stream);
/* The PLY records of a mesh that is already on the HOST (trimesh.Trimesh(vertices, faces, vertex_colors).export(), trainer_generic.py:1302-1303,
 * 1377-1382): vertices fp64 [n,3], colors uint8 [n,3|4] or NULL, faces int64 [m,3], all host pointers -> vertex_records n x (16 | 12) bytes,
 * face_records m x 13 bytes.  Plain host code (up to four threads), no device work, no stream. */
int o2345_ply_records_host(const double* vertices, long long n, const uint8_t* colors, int color_channels, const long long* faces, long long m,
                           uint8_t* vertex_records, uint8_t* face_records);

/* ---- asset export (additive since 2.1; replaces utils/utils.py:31-47, convert_mesh_format: mesh.ply -> trimesh -> re-oriented mesh.glb / mesh.obj) -----
 * Output frame: the reference's two rotations and x flip compose to the exact swap (x, y, z) -> (x, z, y) (z-up -> glTF's y-up), and every face is
 * reversed (a, b, c) -> (c, b, a).  Positions are the float32 positions of o2345_mesh_pack_vertices with columns 1 and 2 exchanged, bit for bit.
 *
 * mesh_asset_vertices (replaces utils/utils.py:34-40): verts_idx, bounds and matrices as for o2345_mesh_pack_vertices; rgb device fp32 [n,3] or NULL;
 * grad device fp32 [n,3] (SDF gradient in the reconstruction frame) or NULL.  Outputs, all device: positions float32 [n,3]; rgba uint8 [n,4] (written
 * iff rgb; truncating quantisation, alpha 255; 4-byte aligned); normals float32 [n,3] (written iff grad): normalize(grad) through the 3x3 of trans_mat
 * when given, renormalised, swapped -- towards increasing SDF; (0, 1, 0) for a zero or non-finite gradient; bounds float32 [6] = per-axis min then max of
 * positions (glTF's POSITION accessor needs them), from a two-stage reduction through `workspace` (o2345_mesh_bounds_workspace_bytes(n) bytes, 4-byte
 * aligned): deterministic, no floating-point atomics.  n = 0 writes nothing. */
size_t o2345_mesh_bounds_workspace_bytes(long long n);
int o2345_mesh_asset_vertices(const double* verts_idx, long long n, int grid_R, const float* bound_min_host, const float* bound_max_host, const float* scale_mat_host,
                              const float* trans_mat_host, const float* rgb, const float* grad, float* positions, uint8_t* rgba, float* normals,
                              float* bounds, void* workspace, size_t workspace_bytes, void* stream);
/* replaces utils/utils.py:41 (np.fliplr(mesh.faces)): tris device int32 / int64 [m,3] (index_bytes 4 / 8) -> indices uint32 [m,3], winding reversed. */
int o2345_mesh_asset_indices(const void* tris, int index_bytes, long long m, uint32_t* indices, void* stream);
/* OBJ text (replaces utils/utils.py:42-44, mesh.export(file_type='obj', include_color=True)): fixed-width ASCII records, n vertex records, then n
 * normal records when normals are given, then m face records; record i of a kind starts at i * its length.
 *   coordinate field " %*.8f", 1 + (1 + K + 1 + 8) bytes, K = integer digits of the largest |coordinate| after rounding to 8 decimals (1 .. 9; the caller
 *   takes it from `bounds`); colour field " %.8f" of c / 255, 11 bytes;
 *   "v" + 3 coordinate fields [+ 3 colour fields] + "\n";  "vn" + 3 x " %11.8f" + "\n";
 *   "f" + 3 x " %*d" + "\n" (1-based, width = decimal digits of n), or with normals 3 x " a//a", each token right-aligned in 2 * digits(n) + 2 bytes.
 * Digits are printf's: correctly rounded, ties to even, "-0.00000000" for a negative value that rounds to zero.
 * obj_text_bytes: the byte count (HOST function; 0 for K outside 1 .. 9).  obj_text: positions / rgba (or NULL) / normals (or NULL) / indices as written by
 * the two entries above, all device; color_table device uint8 [256,11], entry c = " %.8f" % (c / 255.0) (needed iff rgba); text device uint8
 * [obj_text_bytes], any alignment.  Indices must be < n. */
size_t o2345_obj_text_bytes(long long n, long long m, int K, int colors, int normals);
int o2345_obj_text(const float* positions, const uint8_t* rgba, const float* normals, long long n, const uint32_t* indices, long long m, int K,
                   const uint8_t* color_table, uint8_t* text, void* stream);
/* The same text for a mesh that is already on the HOST (what convert_mesh_format does after trimesh.load_mesh, utils/utils.py:31-47): host pointers in the
 * layouts above, text host uint8 [obj_text_bytes].  Plain host code (up to four threads), no device work, no stream. */
int o2345_obj_text_host(const float* positions, const uint8_t* rgba, const float* normals, long long n, const uint32_t* indices, long long m, int K,
                        uint8_t* text);
/* ---- texture atlas of the exported mesh (additive since 2.1; none in the reference: its assets carry vertex colours only, trainer_generic.py:1377-1382,
 * utils/utils.py:31-47) ------------------------------------------------------------------------------------------------------------------------------
 * Layout for nt >= 1 triangles and texel = c in [4, 64], the edge of a cell in texels: triangles 2k and 2k + 1, in face order, share square cell k;
 * cells = ceil(nt / 2), G = ceil(sqrt(cells)); cell k sits at column k mod G, row k div G; the image is W = G c wide, H = ceil(cells / G) c high, row 0
 * on top.  Refused: W or H over 16384, cells c^2 >= 2^31.  Local texel (i, j) of a cell has its centre at (i + 0.5, j + 0.5).  Triangle A = 2k has its
 * corners at local uv (0.5, 0.5), (c - 1.5, 0.5), (0.5, c - 1.5) and owns the texels with i + j <= c - 1; triangle B = min(2k + 1, nt - 1) has them at
 * (c - 0.5, c - 0.5), (2.5, c - 0.5), (c - 0.5, 2.5) and owns those with i + j >= c (for an odd nt the B half of the last cell repeats the last
 * triangle).  A bilinear fetch (texel centres at + 0.5, clamp to edge, no mipmaps) anywhere in a triangle reads only texels that triangle owns.
 * mesh_texture_texels (HOST function): cells c^2, the length of the texel lists, and W, H through the two host pointers (either may be NULL); 0 for a
 * refused layout.
 * mesh_texture_points: the surface point of every texel of every used cell, cell-major (entry k c^2 + j c + i).  Barycentric weights of the centre with
 * respect to the owner's uv corners -- A: w1 = i / (c - 2), w2 = j / (c - 2); B: w1 = (c - 1 - i) / (c - 3), w2 = (c - 1 - j) / (c - 3); w0 = (1 - w1)
 * - w2; never clamped: gutter texels extrapolate -- then p = (w0 P0 + w1 P1) + w2 P2 on the index-space corners, each coordinate clamped to [0, R - 1],
 * and the world point float32(p / (R - 1) * ext + bmin) as o2345_mesh_project defines it; fp64, one operation at a time, in the order written: equal to
 * mesh_io.texture_points to the last bit.  verts device fp64 [nv,3], tris device int32 / int64 [nt,3] (index_bytes 4 / 8), both only read; 1 <= nv <
 * 2^30; bound_min / bound_max HOST float32 [3], bound_max > bound_min.  Outputs, device: points_idx fp64 [texels,3], points_world float32 [texels,3],
 * stats (8-byte aligned), written by this call.  An index outside [0, nv) is read as vertex 0, never dereferenced; a non-zero counter means bad input
 * and the caller raises.  No host synchronisation.
 * mesh_texture_pack: rgb device fp32 [texels,3] in the order above -> image device uint8 [H,W,4], 4-byte aligned, raster order: the truncating
 * quantisation of the vertex colours, alpha 255; texels of unused cells are 0, 0, 0, 0.
 * mesh_texture_corners: the unwelded vertices.  Triangle t = (a, b, c) gives vertices 3t, 3t + 1, 3t + 2 = c, b, a (the asset frame's reversed winding):
 * positions float32 [3 nt,3] = that vertex's position of o2345_mesh_asset_vertices, bit for bit; uv float32 [3 nt,2] = ((cell_x c + u_local) / W,
 * (cell_y c + v_local) / H), fp64 rounded once; normals float32 [3 nt,3] (written iff grad, device fp32 [nv,3]) = that vertex's normal of
 * o2345_mesh_asset_vertices; indices uint32 [3 nt] = 0, 1, 2, ...; bounds float32 [6] and workspace (o2345_mesh_bounds_workspace_bytes(3 nt) bytes) as
 * for o2345_mesh_asset_vertices.  Bounds and matrices as for o2345_mesh_pack_vertices. */
typedef struct O2345TextureStats {
    unsigned long long n_nonfinite;                     /* triangles with a non-finite corner coordinate */
    unsigned long long n_bad;                           /* triangles with an index outside [0, nv) */
} O2345TextureStats;
size_t o2345_mesh_texture_texels(long long nt, int texel, int* width_host, int* height_host);
int o2345_mesh_texture_points(const double* verts, long long nv, const void* tris, int index_bytes, long long nt, int texel, int grid_R,
                              const float* bound_min_host, const float* bound_max_host, double* points_idx, float* points_world, O2345TextureStats* stats,
                              void* stream);
int o2345_mesh_texture_pack(const float* rgb, long long nt, int texel, uint8_t* image, void* stream);
int o2345_mesh_texture_corners(const double* verts, long long nv, const void* tris, int index_bytes, long long nt, int texel, int grid_R,
                               const float* bound_min_host, const float* bound_max_host, const float* scale_mat_host, const float* trans_mat_host, const float* grad,
                               float* positions, float* uv, float* normals, uint32_t* indices, float* bounds, void* workspace, size_t workspace_bytes,
                               void* stream);
/* Tangent-space normal map of the textured asset (additive; none in the reference).  Everything is fp64, one operation at a time, in the order written;
 * a dot product is (x x + y y) + z z; square roots and divisions are IEEE: equal to mesh_io.texture_frames / pack_normal_map to the last bit
 * (csrc/mesh_normalmap_math.h is the one spelling of the arithmetic).
 * mesh_texture_frames: one frame per triangle from the file's own buffers, the positions [3 nt,3] and uv [3 nt,2] of mesh_texture_corners (device float32,
 * only read), promoted to fp64.  Triangle t has corners q = 3t, 3t + 1, 3t + 2 with positions p0, p1, p2 and texture coordinates uv0, uv1, uv2: e1 = p1 -
 * p0, e2 = p2 - p0, N = unit(e1 x e2) (the front face of the file's winding); (du1, dv1) = uv1 - uv0, (du2, dv2) = uv2 - uv0, det = du1 dv2 - du2 dv1, Pu =
 * (e1 dv2 - e2 dv1) / det, Pv = (e2 du1 - e1 du2) / det; T = unit(Pu - N (N . Pu)); w = +1 if (N x T) . (-Pv) >= 0, else -1 (green is up, and up is
 * decreasing v: row 0 of the image is on top).  normals device float32 [3 nt,3] = N and tangents device float32 [3 nt,4] (16-byte aligned) = (T, w), the
 * same for the three corners of a triangle (flat).  A triangle is degenerate when |e1 x e2|, det or |Pu - N (N . Pu)| is zero or not finite: it gets N =
 * (0, 1, 0) and tangent (1, -0, 0, 1) and is counted once: the NEGATIVE zero of its y is the value of the definition and the mark of a degenerate
 * triangle; a sound triangle never carries it, because every float32 component of its N and T has + 0 added, which turns a negative zero into a positive
 * one and changes nothing else (a flat axis-aligned triangle has the frame (0, 1, 0), (1, 0, 0, 1) for good reasons).  1 <= nt < 2^31 / 3.
 * mesh_texture_normal_pack: one RGBA8 texel per image texel, raster order as for mesh_texture_pack; image device uint8 [H,W,4], 4-byte aligned.  A texel
 * of a used cell has its owner triangle t by the A / B rule above (the repeated last triangle of an odd nt included) and its cell-major entry s; grad
 * device float32 [texels,3] is the raw SDF gradient at the texel points.  n = grad[s] through the operations of the asset normals (normalise; through
 * rotation, device float32 [9] = the 3x3 of trans_mat, row-major, or NULL, and renormalise; y and z exchanged), kept in fp64.  With the float32 N, T, w of
 * corner 3t promoted to fp64 and B = w (N x T): x = n . T, y = n . B, z = n . N, each channel clamp(floor((x 127.5 + 127.5) + 0.5), 0, 255), alpha 255.
 * (128, 128, 255, 255) for a texel of an unused cell, for a texel whose triangle carries the degenerate mark above and for a texel whose gradient has a
 * zero or non-finite length, before or behind the rotation.
 * counters: device int64 [4], 8-byte aligned = {degenerate triangles, bad-gradient texels, back-facing texels, reserved}.  mesh_texture_frames zeroes all
 * four and counts the first; mesh_texture_normal_pack zeroes and counts the last three and leaves the first alone, so that one block serves the chain.
 * Bad gradients are counted over every texel of a used cell; back-facing ones (z < 0; informative, not an error) where z is computed.
 * Bad input never faults; no host synchronisation. */
int o2345_mesh_texture_frames(const float* positions, const float* uv, long long nt, float* normals, float* tangents, long long* counters, void* stream);
int o2345_mesh_texture_normal_pack(const float* grad, const float* rotation, const float* normals, const float* tangents, long long nt, int texel,
                                   uint8_t* image, long long* counters, void* stream);
/* The records of the textured OBJ (none in the reference), for n = 3 nt unwelded vertices as written by mesh_texture_corners: n "v" records without
 * colours, n "vt" + 2 x " %10.8f" records (u, then float32(1 - v): OBJ's origin is bottom-left), n "vn" records when normals are given, n / 3 records
 * "f a/a b/b c/c" (with normals "a/a/a") over the corners 1 .. n in order, each token right-aligned in 2 d + 1 (3 d + 2) bytes, d = decimal digits of n.
 * Fields and K as for o2345_obj_text.  obj_texture_text_bytes: the byte count (HOST function; 0 for K outside 1 .. 9 or n not a multiple of 3). */
size_t o2345_obj_texture_text_bytes(long long n, int K, int normals);
int o2345_obj_texture_text(const float* positions, const float* uv, const float* normals, long long n, int K, uint8_t* text, void* stream);
/* ---- surface render (additive since 2.1; none in the reference: models/fast_renderer.py calls sdf_from_sdfvolume with a keyword it does not accept) ----
 * Depth, hit point and kind per ray by an exhaustive fixed-stride march through the TRILINEAR R^3 lattice u (device float32 [R,R,R], x-major, 2 <= R <=
 * 2048), equal to the host twin (surface.py) to the last bit: fp64, one operation at a time, in the order written, no square root in the trace.
 *   field    g(node) = double(u) - level, or level - double(u) with inside_positive (the extraction lattice is -sdf); a value is OUTSIDE iff it is > 0.
 *   bricks   8 x 8 x 8 cells, nb = ceil((R - 1) / 8) per axis; surface_bricks writes flags uint8 [nb,nb,nb]: 1 iff some node with index in [8 b_k,
 *            min(8 b_k + 8, R - 1)] on every axis fails g > 0 (a NaN node sets it).
 *   ray      o, d device float32 [n,3] widened; bound_min / bound_max HOST float32 [3] widened, ext = bmax - bmin.  Per axis k with d_k == 0: nothing is
 *            constrained when bmin_k <= o_k <= bmax_k, else the ray misses the box; with d_k != 0: a = (bmin_k - o_k) / d_k, b = (bmax_k - o_k) / d_k,
 *            low = min(a, b), high = max(a, b).  t0 = max(near, lows), t1 = min(far, highs); a ray that fails t0 <= t1 misses the box.  A non-finite o or
 *            d is a BAD ray: counted, never dereferenced.
 *   samples  h = stride * min_k(ext_k) / (R - 1) -- `stride` lattice spacings for a unit direction; h is a step in t, so a non-unit direction scales
 *            it.  n = floor((t1 - t0) / h), n > 2^20 is a bad ray; t_j = t0 + j h (a product) for j = 0 .. n, one more sample at t1 when t_n < t1.
 *   value    p_k = o_k + t d_k; x_k = (p_k - bmin_k) / ext_k * (R - 1), clamped to [0, R - 1] (a NaN clamps to 0); i_k = min(floor(x_k), R - 2), f_k =
 *            x_k - i_k; v = sum over the eight corners of ((wx wy) wz) g(corner), w = f or 1 - f, dx outer, dy, dz inner, from 0, left to right.
 *   skip     with flags given, a sample whose cell lies in a brick with flag 0 is outside without a lookup (exact in floating point: eight corners > 0
 *            give a sum of non-negative products, one of them >= g / 8 > 0); a skipped predecessor is evaluated when a bracket needs it.  flags NULL:
 *            every sample is looked up; the outputs are the same bytes, only the lookup counter differs.
 *   march    j = the first sample that is not outside.  Its value NaN: the ray is STALLED (kind 0, counted).  j = 0: an entry hit at t0, kind 2.  Else
 *            lo = t_{j-1}, hi = t_j and `refine` (0 .. 32) steps tm = lo + (hi - lo) * (s_lo / (s_lo - s_hi)) on even, lo + (hi - lo) * 0.5 on odd
 *            steps; an outside value at tm replaces lo, anything else hi; depth = lo + (hi - lo) * (s_lo / (s_lo - s_hi)), kind 1 (a non-finite depth
 *            -- infinite lattice values -- is stalled).  No such j: a miss, kind 0.
 *   outputs  device: depth float32 [n] = float32(t), 0 without a hit; kind uint8 [n]; point float32 [n,3] = float32(o_k + t d_k), 0 without a hit;
 *            the hit list, int32 at the start of `workspace` (surface_trace_workspace_bytes(n) bytes, 16-byte aligned): the slots with kind != 0, each
 *            once, in an order that changes between runs (ballot compaction, one integer atomicAdd per wave) -- the network kernels take it as `index`
 *            with its device-side count (stats->n_list) as `n_dev`; stats (8-byte aligned), written by this call.
 *   img_h, img_w: 0, 0, or the image the n = img_h img_w rays fill in raster order: a wave then takes an 8 x 8 pixel tile instead of 64 consecutive rays
 *            (lanes of similar march length together); the results are the same bytes.
 * No host synchronisation.  Errors: bad arguments, a workspace that is too small.
 * camera_rays: rays through the pixel grid of a pinhole camera without skew, raster order -- K_host float32 [9] = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]
 * (anything else is refused), c2w_host float32 [12] (rows 0 .. 2 of the 4x4), both HOST.  In fp64: v = ((px - cx) / fx, (py - cy) / fy, 1), divided by
 * sqrt((vx vx + vy vy) + vz vz), rotated by c2w's 3x3 with sums left to right, rounded to float32 once -> rays_d device float32 [H W,3]; rays_o = c2w's
 * translation.
 * surface_pack: kind uint8 [H W], depth float32 [H W], rgb and grad float32 [H W,3] (read at kind != 0 only), raster order -> color uint8 [H,W,4]: the
 * truncating quantisation of the vertex colours, alpha 255, and background_host (HOST uint8 [4]) without a hit; normal uint8 [H,W,4]: that quantisation of
 * float32(n 0.5 + 0.5), n = grad / sqrt((gx gx + gy gy) + gz gz) in fp64 (0 for a zero or non-finite gradient), alpha 255, and 0, 0, 0, 0 without a hit;
 * depth_out float32 [H,W]: depth, 0 without a hit.  The two images are 4-byte aligned. */
typedef struct O2345SurfaceStats {
    unsigned long long hits, entry_hits;
    unsigned long long box_misses, misses;              /* rays that miss the box; rays marched through without a hit */
    unsigned long long stalled, bad_rays;
    unsigned long long samples;                         /* samples visited: march samples + refinement evaluations */
    unsigned long long lookups;                         /* lattice lookups */
    int n_list;                                         /* the hit list's count */
    int reserved;                                       /* 0 */
} O2345SurfaceStats;
int o2345_surface_bricks(const float* u, int grid_R, double level, int inside_positive, uint8_t* flags, void* stream);
size_t o2345_surface_trace_workspace_bytes(long long n);
int o2345_surface_trace(const float* u, int grid_R, const uint8_t* flags, const float* rays_o, const float* rays_d, long long n, int img_h, int img_w,
                        double t_near, double t_far, double stride, int refine, double level, int inside_positive, const float* bound_min_host,
                        const float* bound_max_host, void* workspace, size_t workspace_bytes, float* depth, uint8_t* kind, float* point,
                        O2345SurfaceStats* stats, void* stream);
int o2345_camera_rays(const float* K_host, const float* c2w_host, int H, int W, float* rays_o, float* rays_d, void* stream);
int o2345_surface_pack(const uint8_t* kind, const float* depth, const float* rgb, const float* grad, int H, int W, const uint8_t* background_host,
                       uint8_t* color, uint8_t* normal, float* depth_out, void* stream);
/* ---- mesh-to-mesh distance (additive since 2.1; none in the reference: its meshes are never compared as surfaces) ----------------------------------------
 * Everything is fp64, one operation at a time, in the order written, a dot product (x x + y y) + z z; equal to the host twin (mesh_io.surface_samples,
 * closest_triangles) to the last bit.  verts device fp64 [nv,3], tris device int32 / int64 [nt,3] (index_bytes 4 / 8), both only read; 0 <= nv < 2^30,
 * 3 * nt < 2^31.  Workspaces and the grid object are 16-byte aligned; every *_bytes function returns 0 for bad sizes.
 *   samples   triangle t (corners P0, P1, P2) at `spacing` (finite, > 0; 0 = one sample per triangle): L2 = the largest squared edge length, k_t = the
 *             smallest k in [1, 64] with (k spacing)(k spacing) >= L2, 64 if there is none (1 without a spacing).  The triangle is split regularly into
 *             k^2 sub-triangles and sampled at their centroids: the upright ones first, j = 0 .. k - 1, i = 0 .. k - 1 - j: w1 = (3 i + 1) / (3 k), w2 =
 *             (3 j + 1) / (3 k); then the inverted ones, j = 0 .. k - 2, i = 0 .. k - 2 - j: w1 = (3 i + 2) / (3 k), w2 = (3 j + 2) / (3 k); w0 = (1 - w1)
 *             - w2, p = (w0 P0 + w1 P1) + w2 P2.  Weight: area_t / k^2, area_t = 0.5 sqrt(n . n), n = (P1 - P0) x (P2 - P0).  Samples are numbered
 *             triangle-major.  samples_count returns their number on the HOST (synchronises the stream once); errors: 2^28 samples or more, a non-finite
 *             coordinate, an index outside [0, nv) -- counted on the device, never dereferenced.  samples_emit (same workspace, nv, nt, untouched in
 *             between; n_samples as counted) writes points fp64 [n,3], weights fp64 [n], triangle int32 [n]; any of the three may be NULL.
 *   d2        squared distance from p to triangle (A, B, C): |p - q|^2, q from the region walk of Ericson, Real-Time Collision Detection 5.1.5, regions
 *             tested in the book's order (csrc/mesh_distance_math.h, md_point_triangle, is the text).  A target triangle is USABLE iff its indices are in
 *             range, its coordinates finite and n . n != 0.  d2 [i] = the minimum over the usable triangles, nearest [i] = the smallest index that
 *             attains it; +inf and -1 without a usable triangle.
 *   grid      a uniform grid of cells of edge `cell` (finite, > 0; 0 = the default: about as many cells as usable triangles) aligned to the multiples of
 *             the edge, over the bounds of the usable triangles; an edge that gives more than 256 cells along an axis or more than max_cells (1 .. 2^24)
 *             in all is enlarged by factors of 1.25.  Every usable triangle is listed in each cell its bounding box touches; a list is ascending.
 *             grid_count returns on the HOST (one synchronisation) the number of list entries, and optionally the degenerate triangles, the cells per
 *             axis and the edge in use; errors as for samples, plus a target without a usable triangle, plus 2^31 entries or more.  grid_emit (same
 *             workspace and arguments, n_entries as counted) writes the grid object: grid_bytes(max_cells, n_entries) bytes.
 *   query     points device fp64 [n,3], n < 2^28 -> d2 fp64 [n], nearest int32 [n].  grid NULL: every point against every triangle.  grid given (with
 *             the max_cells it was built with, over the same verts and tris): the same bits through the grid -- shells of cells outward from the
 *             point's cell, stopping when a conservative lower bound on the distance to everything unvisited exceeds the best distance found.
 *   reduce    d2, nearest (may be NULL), weights (NULL = 1) over n samples; thresholds HOST fp64 [n_thresholds <= 8], finite and >= 0 -> stats,
 *             8-byte aligned (d = sqrt(d2); the target is optional, tris NULL = none).  The sums are the same bits on every run (fixed tree, no
 *             floating-point atomics; at most 288 additions in a chain).  No host synchronisation. */
typedef struct O2345DistanceStats {
    double sum_w, sum_wd, sum_wd2;                      /* sum w, sum w d, sum w d^2 */
    double within[8];                                   /* sum w [d <= tau_k] */
    unsigned long long max_d2_bits;                     /* the bit pattern of the largest d2 */
    unsigned long long n;
    unsigned long long n_unmatched;                     /* the samples left out: d2 not finite or negative, or nearest < 0 */
    unsigned long long n_degenerate, n_bad;             /* of the target: degenerate triangles; those with a bad index or a non-finite coordinate */
} O2345DistanceStats;
size_t o2345_mesh_samples_workspace_bytes(long long nt);
int o2345_mesh_samples_count(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, double spacing, void* workspace,
                             size_t workspace_bytes, long long* n_samples_host, void* stream);
int o2345_mesh_samples_emit(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, void* workspace, long long n_samples,
                            double* points, double* weights, int* triangle, void* stream);
size_t o2345_mesh_distance_grid_workspace_bytes(long long nt, long long max_cells);
size_t o2345_mesh_distance_grid_bytes(long long max_cells, long long n_entries);
int o2345_mesh_distance_grid_count(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, double cell, long long max_cells,
                                   void* workspace, size_t workspace_bytes, long long* n_entries_host, long long* n_degenerate_host, int* dims_host,
                                   double* cell_host, void* stream);
int o2345_mesh_distance_grid_emit(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, long long max_cells, void* workspace,
                                  long long n_entries, void* grid, size_t grid_bytes, void* stream);
int o2345_mesh_distance_query(const double* points, long long n, const double* verts, const void* tris, int index_bytes, long long nv, long long nt,
                              const void* grid, size_t grid_bytes, long long max_cells, double* d2, int* nearest, void* stream);
size_t o2345_mesh_distance_reduce_workspace_bytes(long long n);
int o2345_mesh_distance_reduce(const double* d2, const int* nearest, const double* weights, long long n, const double* thresholds_host, int n_thresholds,
                               const double* verts, const void* tris, int index_bytes, long long nv, long long nt, void* workspace, size_t workspace_bytes,
                               O2345DistanceStats* stats, void* stream);

/* ---- mesh alignment (additive since 2.3.1; the reference aligns its meshes in another tool before it reports an F-score) --------------------------------
 * One step of aligning mesh A to mesh B by a similarity transform: the moments of the point-to-plane Gauss-Newton system of A's samples against B, for
 * n_transforms (1 .. 64) candidate transforms at once.  The 7 x 7 solve and the loop are the caller's (mesh_io.similarity_step, align_meshes).  Everything
 * is fp64, one operation at a time, in the order written (csrc/mesh_align_math.h is the text), equal to the host twin (mesh_io.align_terms) to the last bit
 * per sample.  points device fp64 [n,3], weights device fp64 [n] (NULL = 1), n < 2^28; transforms device fp64 [n_transforms,12], the rows of [M | t].
 *   pair      (transform k, sample e): x = M_k p_e + t_k, x_i = ((M_i0 p_0 + M_i1 p_1) + M_i2 p_2) + t_i; d2 and nearest of x are those of
 *             o2345_mesh_distance_query over the same verts, tris and grid (grid NULL: every triangle), bit for bit; q is the closest point of triangle
 *             `nearest` (A, B, C).  MATCHED: nearest >= 0 and d2 finite and >= 0.  INLIER: matched and (max_distance == 0 or d2 <= max_distance^2).
 *   terms     x' = x - pivot, n = ((B - A) x (C - A)) / sqrt(n . n), J = (x' x n, n, n . x') (seven entries), b = n . (q - x): (w J_i) J_j for i <= j and
 *             (w J_i) b.
 *   moments   device fp64 [n_transforms,48], per transform: 0 .. 27 the upper triangle of sum w J J^T, row-major; 28 .. 34 sum w J b; 35 sum w and 36
 *             sum w d2 (all over the inliers); 37 sum w and 38 sum w min(d2, max_distance^2) over the matched (max_distance == 0: sum w d2); 39 .. 41
 *             sum w x' and 42 sum w |x'|^2 over the inliers; 43, 44, 45 the numbers of inliers, of matched samples that are no inliers, and of unmatched
 *             samples, as doubles; 46, 47 zero.  The sums are the same bits on every run (the tree of o2345_mesh_distance_reduce per transform, at most
 *             288 additions in a chain, no floating-point atomics).
 *   tris NULL no target: every sample is an inlier with q = x and d2 = 0 and columns 0 .. 34 are 0 -- columns 35 and 39 .. 42 give the centroid and the rms
 *             radius of a sample set; with `moved` it is the transform of a point set.
 *   outputs   moved fp64 [n_transforms,n,3], d2 fp64 [n_transforms,n], nearest int32 [n_transforms,n]: each may be NULL, and nothing of that size is
 *             written without them.
 * Errors: bad sizes, max_distance negative or not finite, a pivot or a transform entry that is not finite (the transforms are read back to check them: one
 * synchronisation of the stream).  A target index out of range or a non-finite target coordinate is skipped as the query skips it.
 * workspace_bytes(n, n_transforms) is 0 for n < 0, n >= 2^28, n_transforms < 1 or > 64. */
size_t o2345_mesh_align_workspace_bytes(long long n, int n_transforms);
int o2345_mesh_align_step(const double* points, const double* weights, long long n, const double* transforms, int n_transforms, const double* verts,
                          const void* tris, int index_bytes, long long nv, long long nt, const void* grid, size_t grid_bytes, long long max_cells,
                          double max_distance, double pivot_x, double pivot_y, double pivot_z, void* workspace, size_t workspace_bytes, double* moments,
                          double* moved, double* d2, int* nearest, void* stream);

/* ---- simplification by quadric-error edge collapse (additive since 2.2; the reference has no such step, its users simplify the mesh in another tool) ----
 * Rounds of independent half-edge collapses ordered by Garland - Heckbert's quadric error, subset placement: collapsing v -> u removes v, u keeps its
 * bits, positions never change.  Everything is fp64, one operation at a time, in the order written (csrc/mesh_simplify_math.h is the text); equal to
 * mesh_io.simplify_mesh to the last bit.  Triangle quadric, once, from the input: n = (P1 - P0) x (P2 - P0), nn = (nx nx + ny ny) + nz nz; nn > 0: s = 0.5 /
 * sqrt(nn), d = -((nx P0x + ny P0y) + nz P0z), the ten entries (a b) s over (nx, ny, nz, d); else zeros.  Q_v = the sequential entrywise sum over the
 * triangles of v in ascending face order; after a collapse Q_u <- Q_u + Q_v.  A round, on its live triangles, N(v) the adjacency row of v: the half-edge
 * v -> u is eligible iff (1) every edge at v has exactly two triangles (boundary vertices and vertices on non-manifold edges are never removed, though they
 * may be targets), (2) |N(v) & N(u)| = 2, (3) for every triangle at v without u the normal n' after replacing P_v by P_u has n . n' > 0 against the old
 * normal, (4) e = p^T (Q_v + Q_u) p at p = P_u is finite and cost = max(0, e) <= max_error.  Candidate of v: its eligible u of least cost, ties to the
 * smaller u.  With C candidates and need = ceil((live - target_faces) / 2): bin(cost) = the biased exponent field of the double, B = the smallest bin whose
 * cumulative count reaches max(1, min(8 need, ceil(C / 2))); the candidates with bin <= B take part, priority (splitmix64's finaliser of v + (round << 32),
 * v).  v is selected iff its priority is the smallest among the participants within graph distance 2; all selected collapses apply at once; triangles
 * with two equal corners are dropped; face order, corner order and orientation stay.  Stop: live <= target_faces (TARGET), no candidate (BLOCKED),
 * max_rounds rounds done (ROUNDS); the last round may go below the target.  A vertex is kept iff a kept triangle references it, in the old order; triangles
 * are renumbered by an exclusive scan.  Not done: optimal placement, boundary and non-manifold collapses, a valence cap, an exact hit of the target.
 * verts device fp64 [nv,3], tris device int32 / int64 [nt,3] (index_bytes 4 / 8), both only read; 0 <= nv < 2^30, 6 * nt < 2^31; target_faces >= 0;
 * max_error >= 0, infinity = no limit; max_rounds >= 0.  workspace: mesh_simplify_workspace_bytes(nv, nt) bytes (0 for bad sizes), 16-byte aligned.
 * stats: device, sizeof(O2345SimplifyStats) + 8 * max_rounds bytes, 8-byte aligned, written by count(): the struct, then long long collapses[max_rounds],
 * the collapses of every round.  The caller reads the two sizes from it to allocate the outputs.  count() runs all rounds inside the workspace; it
 * synchronises the stream once after the input check and once per round.  Errors: bad arguments, a workspace that is too small, a non-finite coordinate, a triangle index outside [0, nv), a
 * triangle with a repeated index; the last three are counted on the device, never dereferenced.  emit() (same workspace, nv and nt, untouched in
 * between) writes verts_out device fp64 [vertices,3] (bit copies), tris_out [triangles,3] of width index_bytes, source device int32 [vertices] (new ->
 * old) and merged device int32 [nv] (the new index of the vertex each old vertex ended in, following the collapses, or -1); any of the four may be NULL. */
typedef struct O2345SimplifyStats {
    long long rounds;                                   /* rounds that applied collapses */
    long long vertices, triangles;                      /* of the output */
    long long stopped;                                  /* one of the three codes below */
    unsigned long long max_cost_bits;                   /* the bit pattern of a non-negative double: the largest cost applied; 0 without a collapse */
    long long reserved[3];                              /* 0 */
} O2345SimplifyStats;                                   /* behind it in the same buffer: long long collapses[max_rounds], entry r the collapses of round r */
enum { O2345_SIMPLIFY_STOPPED_TARGET = 0, O2345_SIMPLIFY_STOPPED_BLOCKED = 1, O2345_SIMPLIFY_STOPPED_ROUNDS = 2 };        /* the values of `stopped` */
size_t o2345_mesh_simplify_workspace_bytes(long long nv, long long nt);
int o2345_mesh_simplify_count(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, long long target_faces, double max_error,
                              int max_rounds, void* workspace, size_t workspace_bytes, O2345SimplifyStats* stats, void* stream);
int o2345_mesh_simplify_emit(const double* verts, int index_bytes, long long nv, long long nt, void* workspace, double* verts_out, void* tris_out, int* source,
                             int* merged, void* stream);

/* ---- audit of a mesh: manifoldness, orientation, element quality (additive since 2.2; none in the reference: its meshes are never checked) -------------
 * Read-only; equal to the host twin mesh_io.mesh_audit: integers, flags, quality, minima and maxima to the last bit, the three sums to 1e-12 of the sum of
 * their terms' magnitudes.  Everything is fp64, one operation at a time, in the order written (csrc/mesh_audit_math.h is the text), a dot product (x x + y y)
 * + z z.  verts device fp64 [nv,3], tris device int32 / int64 [nt,3] (index_bytes 4 / 8), both only read; 0 <= nv < 2^30, 6 * nt < 2^31.
 *   triangles  two equal indices: REPEATED, counted, flagged, no part in anything else.  The others (FACES): n = (P1 - P0) x (P2 - P0), nn = n . n, ZERO_AREA iff
 *              nn == 0; area_t = 0.5 sqrt(nn); v_t = P0 . (P1 x P2); l01, l12, l20 the squared edge lengths, s = (l01 + l12) + l20; quality q_t =
 *              (6.928203230275509 area_t) / s (4 sqrt 3: 1 for an equilateral triangle), 0 when s == 0.  Histogram: bin min(9, floor(q 10)); a q that is not
 *              >= 0 enters no bin and no minimum.
 *   edges      half-edge 3 t + i runs from tris[t][i] to tris[t][(i + 1) % 3]; the undirected edge {lo, hi} has m half-edges, of which some run lo -> hi.
 *              BOUNDARY m = 1, manifold m = 2, NONMANIFOLD m >= 3; a manifold edge is INCONSISTENT iff both half-edges run the same way; a manifold,
 *              consistent edge whose two triangles have nn > 0 is CREASED iff n . n' < 0 (a right angle is not).
 *   vertices   used: referenced by a face; boundary: on a boundary edge; non-manifold: on an edge with m >= 3.  Fans: over the corners (t, i) of the
 *              faces, every manifold edge {u, w}, whatever its orientation, joins the two corners at u and the two corners at w; fans(v) = the classes
 *              among the corners at v.  BOWTIE iff fans(v) >= 2 and v lies on no non-manifold edge.
 *   sums       area = sum area_t, sum v_t (six times the volume of a closed, consistent mesh), sum q_t: every block folds its 256 triangles in a fixed
 *              tree, one block folds the rows; the same bits on every run, no floating-point atomics.  min q_t, min and max squared edge length over the
 *              faces' half-edges; without a face the two minima are +inf and the maximum is 0.
 * stats: device, 8-byte aligned, written by this call.  vertex_flags uint8 [nv]: bit 0
 * boundary, 1 on a non-manifold edge, 2 bow-tie, 3 unused.  face_flags uint8 [nt]: bit 0 repeated, 1 zero-area, 2 has a boundary edge, 3 a non-manifold
 * edge, 4 an inconsistent edge, 5 a creased edge.  quality fp64 [nt]: 0 for a repeated triangle.  Any of the three may be NULL.  A triangle index outside
 * [0, nv) and a vertex with a non-finite coordinate are counted (bad_index, nonfinite), never dereferenced; the caller reads the two counts and treats
 * the rest as void when one is not 0.  workspace: mesh_audit_workspace_bytes(nv, nt) bytes (0 for bad sizes), 16-byte aligned.  No host synchronisation.
 * Not done: duplicate faces, per-component reports, dihedral statistics, any repair (the hole filling below closes the
 * boundary loops it reports). */
typedef struct O2345AuditStats {
    unsigned long long bad_index, nonfinite;            /* triangles with an index outside [0, nv); vertices with a non-finite coordinate */
    unsigned long long vertices, edges, faces;          /* used vertices, undirected edges, non-repeated triangles */
    unsigned long long repeated_faces, zero_area_faces;
    unsigned long long boundary_edges, nonmanifold_edges, inconsistent_edges, creased_edges;
    unsigned long long boundary_vertices, nonmanifold_vertices, bowtie_vertices, unused_vertices;
    unsigned long long reserved;                        /* 0 */
    unsigned long long histogram[10];                   /* the ten quality bins */
    double area, volume6, quality_sum;                  /* the three sums */
    double quality_min, edge2_min, edge2_max;           /* the smallest quality, the smallest and the largest squared edge length */
} O2345AuditStats;
size_t o2345_mesh_audit_workspace_bytes(long long nv, long long nt);
int o2345_mesh_audit(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, void* workspace, size_t workspace_bytes,
                     O2345AuditStats* stats, unsigned char* vertex_flags_or_null, unsigned char* face_flags_or_null, double* quality_or_null, void* stream);

/* ---- hole filling: closes the boundary loops of a mesh (additive since 2.3; none in the reference: its users close the mesh in another tool) --------------
 * Equal to the host twin mesh_io.fill_holes to the last bit.  verts device fp64 [nv,3], tris device int32 / int64 [nt,3] (index_bytes 4 / 8), both only
 * read; max_edges in [3, 2^31).
 *   half-edges h = 3 t + i runs from tris[t][i] to tris[t][(i + 1) % 3].  A triangle with two equal indices takes no part and is copied through.  The
 *              undirected edge {lo, hi} has m half-edges; a half-edge is a BOUNDARY half-edge iff m == 1.
 *   next       a vertex is SIMPLE iff exactly one boundary half-edge leaves it and exactly one enters it.  For a boundary half-edge h that enters a simple
 *              vertex b, next(h) is the boundary half-edge that leaves b; otherwise next(h) is undefined.  next is injective where it is defined: the boundary
 *              half-edges fall into disjoint cycles and chains.  A chain ends at a vertex that is not simple (a bow-tie on the rim, a non-manifold edge,
 *              inconsistently oriented neighbours) and is left open.
 *   holes      a HOLE is a cycle; its leader is its smallest half-edge, a half-edge's rank its distance from the leader along next, L its number of
 *              half-edges (>= 3).  Holes are ordered by ascending leader.
 *   fill       iff L <= max_edges, with o_k the origin of the hole's half-edge of rank k.  L == 3: one triangle (o_0, o_2, o_1), no new vertex.  L >= 4:
 *              one new vertex c, per coordinate acc = 0, acc = acc + P[o_k] for k = 0 .. L - 1 in rank order (one sequential fp64 sum), c = acc / L, and
 *              the L triangles (o_{k+1 mod L}, o_k, c) in rank order.  Every new triangle carries the half-edge opposite to the one it closes: an oriented
 *              input stays oriented.
 *   output     verts_out [nv_out,3] = verts bit for bit and in order, then the new vertices in hole order; tris_out [nt_out,3] (the input's width) = tris
 *              unchanged and in order, then the new triangles in hole order, then rank order; hole int32 [nt_out - nt]: for every new triangle the number
 *              of its hole among the filled holes.
 * Two calls (the protocol of the components and the decimation): _count does all the topology inside the workspace (mesh_fill_workspace_bytes(nv, nt)
 * bytes, 0 for bad sizes; 16-byte aligned) and writes counts, device int64 [8], 8-byte aligned: boundary half-edges, holes, filled holes, holes left
 * because L > max_edges, boundary half-edges on chains, the longest hole, nv_out and nt_out -- the caller copies them to the host and allocates the
 * outputs.  It synchronises the stream once, for the refusals that only the device can count: they are its status.  _emit writes the outputs from the same workspace, untouched
 * in between; any output may be NULL.  A triangle index outside [0, nv) is counted on the device, never dereferenced, and fails _count; sizes beyond
 * nv_out < 2^30 or 3 * nt_out < 2^31 are refused.  The pointer-doubling rounds are counted by the host before the first is launched; no floating-point
 * atomics; the same bytes on every run.  A centroid fan is exact for a planar, star-shaped outline and may fold over itself for others (the mesh is
 * combinatorially closed all the same).  Not done: ear clipping or minimum-area triangulation, refinement and fairing of the patch, holes with islands,
 * fixing the vertices that are not simple. */
size_t o2345_mesh_fill_workspace_bytes(long long nv, long long nt);
int o2345_mesh_fill_count(const void* tris, int index_bytes, long long nv, long long nt, long long max_edges, void* workspace, size_t workspace_bytes,
                          long long* counts, void* stream);
int o2345_mesh_fill_emit(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, void* workspace,
                         double* verts_out, void* tris_out, int* hole, void* stream);
/* ---- self-intersections of a mesh: which pairs of triangles cross (additive since 2.3; none in the reference: its users find out in another tool) ---------
 * Read-only; equal to the host twin mesh_io.mesh_intersections to the last bit: counts, per-face hits and the pair list.  Everything is fp64, one operation
 * at a time, in the order written (csrc/mesh_intersect_math.h is the text); only comparisons decide.  verts device fp64 [nv,3], tris device int32 / int64
 * [nt,3] (index_bytes 4 / 8), both only read; 0 <= nv < 2^30, 3 * nt < 2^31.
 *   orient     orient(A, B, C, D): a = A - D, b = B - D, c = C - D; X = b_y c_z - b_z c_y, Y = b_z c_x - b_x c_z, Z = b_x c_y - b_y c_x; the value is
 *              (a_x X + a_y Y) + a_z Z.
 *   crossing   the segment PQ crosses the triangle (A, B, C) iff, with sP = orient(A,B,C,P) and sQ = orient(A,B,C,Q), (sP > 0 and sQ < 0) or (sP < 0 and
 *              sQ > 0), and orient(P,Q,A,B), orient(P,Q,B,C), orient(P,Q,C,A) are all > 0 or all < 0.  A zero or a NaN anywhere: no crossing.
 *   faces      a triangle TAKES PART iff its indices lie in [0, nv), its coordinates are finite, n . n != 0 for n = (P1 - P0) x (P2 - P0) (the grid's
 *              "usable") and its three indices are distinct; the others are skipped and counted.
 *   candidates a pair t < u of faces that take part whose closed bounding boxes overlap on every axis (lo_t <= hi_u and lo_u <= hi_t) and that share at most
 *              one vertex INDEX.  Pairs that share an edge are never tested: a fold along an edge is the audit's "creased".
 *   pairs      a candidate intersects iff for (X, Y) = (t, u) or (u, t) and some i in 0, 1, 2 the edge (X[i], X[(i + 1) % 3]), neither of whose indices is
 *              an index of Y, crosses Y, Y's corners in stored order.
 * grid: the grid object of o2345_mesh_distance_grid_emit over the same verts and tris, with its size and the max_cells it was built with; two overlapping
 * boxes both contain the point max(lo_t, lo_u), so a pair is handled in the one cell that holds that point, by one thread per grid entry against the
 * later entries of its ascending row.  grid NULL: every t against every u > t, for nt <= 2^16; the same bytes either way, and whatever the cell edge.
 * Two calls.  _count (workspace: mesh_intersect_workspace_bytes(nv, nt) bytes, 0 for bad sizes; 16-byte aligned) writes counts, device int64 [8], 8-byte
 * aligned: triangles with an index outside [0, nv), triangles with a non-finite coordinate, faces that take part, faces skipped, candidates, pairs, faces
 * in at least one pair, the most pairs one face is in -- the caller copies them; when one of the first two is not 0 the rest is void (such triangles are
 * counted, never dereferenced, and take no part).  face_hits_or_null: device int32 [nt], the pairs each face is in.  No host synchronisation.  _emit (same
 * arguments and workspace, untouched in between; n_pairs as counted, below 2^30) writes pairs, device int32 [n_pairs,2]: t < u, sorted lexicographically;
 * the same bytes on every run.  Integer atomics only; no kernel waits for another workgroup.
 * Not counted, not done: coplanar overlap and contacts that only touch (a zero determinant is no crossing); a closed component nested inside another
 * without crossing it; the unfiltered fp64 determinant may take the wrong sign next to a degeneracy (the twin takes the same one); coincident vertices
 * with different indices (an unwelded mesh) touch without being counted; no repair. */
size_t o2345_mesh_intersect_workspace_bytes(long long nv, long long nt);
int o2345_mesh_intersect_count(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, const void* grid, size_t grid_bytes,
                               long long max_cells, void* workspace, size_t workspace_bytes, long long* counts, int* face_hits_or_null, void* stream);
int o2345_mesh_intersect_emit(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, const void* grid, size_t grid_bytes,
                              long long max_cells, void* workspace, long long n_pairs, int* pairs, void* stream);
/* ---- mesh rasterizer: depth, barycentrics, face id, colour and normal per pixel of a mesh (additive since 2.3; none in the reference: its meshes are
 * rendered offline in another program) ----
 * Equal to the host twin one-2-3-45_amd/raster.py to the last bit.  All real arithmetic is fp64, one operation at a time, in the order written
 * (csrc/mesh_raster_math.h is the text); coverage is decided in integers.  verts device fp64 [nv,3] in the world frame, tris device int32 / int64 [nt,3]
 * (index_bytes 4 / 8), both only read; 0 <= nv < 2^30, 3 * nt < 2^31; nt = 0 is legal and gives an empty image.
 *   camera     o2345_camera_rays' one, passed the same way: K_host float32 [9] = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] and c2w_host float32 [12] (the 3 x 4,
 *              row-major) on the host, widened to fp64; here fx, fy > 0 and the 3 x 3 of c2w is a rotation (|R^T R - I| <= 1e-5 in every entry).  x right,
 *              y down, z forward; the sample of pixel (px, py) is the integer point (px, py), without a half-pixel offset.  H, W >= 1, H W < 2^31; near
 *              finite and > 0.
 *   corners    a face's corners are renumbered for the computation: corner 0 is the stored corner with the smallest vertex index, the others follow in
 *              stored (cyclic) order, so that the result does not depend on which corner a face is stored from.  Outputs are in STORED order.
 *   screen     q = p - t; x_c = (R00 q_x + R10 q_y) + R20 q_z, y_c with column 1 of R, z_c with column 2; X = x_c / z_c * fx + cx,
 *              Y = y_c / z_c * fy + cy; snapped to 1/256 pixel: sx = (int64) floor(X * 256 + 0.5), sy likewise.
 *   classes    a face is skipped, and counted under the first of these that applies: an index outside [0, nv) (never dereferenced); a non-finite
 *              coordinate; a corner that fails z_c >= near (there is NO clipping: the scenes sit in a unit cube with the camera outside); a corner that
 *              fails |X| <= 2^21 and |Y| <= 2^21 (so that every int64 product stays below 2^61); A2 = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) == 0 on
 *              the snapped integers; culled (cull 0 none, 1 back faces, 2 front faces; a face is FRONT iff A2 < 0: with y down, a triangle whose
 *              (P1 - P0) x (P2 - P0) points at the camera has A2 < 0); the pixel box [ceil(min sx / 256), floor(max sx / 256)] x [the same of sy], clipped
 *              to the image, is empty.
 *   coverage   integers only.  When A2 < 0, corners 1 and 2 are exchanged for the computation (A2 > 0 afterwards).  With a = corner (i + 1) % 3,
 *              b = corner (i + 2) % 3, d = b - a and P = (256 px, 256 py): w_i = d_x (P_y - a_y) - d_y (P_x - a_x), so w0 + w1 + w2 = A2.  The pixel is
 *              covered iff for every i: w_i > 0, or w_i == 0 and (d_y > 0, or d_y == 0 and d_x < 0).  The tie rule accepts exactly one of d and -d: a
 *              pixel on an edge shared by two faces that do not overlap on the screen belongs to exactly one of them, however the mesh is oriented.
 *   depth      l_i = double(w_i) / double(A2); u_i = l_i / z_i with the z_c of the unsnapped corner; iz = (u_0 + u_1) + u_2; z = 1 / iz; b_i = u_i * z.
 *              A face whose z fails z < inf does not cover the pixel.
 *   visibility the covering face with the smallest z wins, by fp64 comparison; ties go to the smaller face index.  The result does not depend on face
 *              order, binning, tile size or run.
 *   outputs    face int32 [H,W] (-1 without a hit); depth float32 [H,W]: z, or with ray_depth z * sqrt((vx vx + vy vy) + 1) for v = ((px - cx) / fx,
 *              (py - cy) / fy, 1), the t of the ray of camera_rays through the pixel (0 without a hit); bary float32 [H,W,3] in stored corner order (0
 *              without a hit).
 *   shading    from face and the float32 bary widened to fp64, corners in stored order: rgb = (b0 c0 + b1 c1) + b2 c2, rounded to float32 once, of the
 *              vertex colours float32 [nv,3] (0.5 without them); nrm the same of the vertex normals float32 [nv,3], or without them the flat
 *              (P1 - P0) x (P2 - P0) of the fp64 vertices; kind uint8 1 at a hit; all 0 without one.  o2345_surface_pack turns kind, depth, rgb and nrm
 *              into images: the colour quantisation, the normal encoding and the background are the surface renderer's.
 * counts: device int64 [O2345_RASTER_COUNTS], 8-byte aligned, read by the enumerators below: the faces skipped by class, the faces binned (that take
 * part), the (tile, face) pairs over 8 x 8-pixel tiles (a face is listed in every tile its pixel box touches) and the covered pixels.
 * Three calls.  _count (workspace: mesh_raster_workspace_bytes(nv, nt, H, W) bytes, 0 for bad sizes; 16-byte aligned) writes every count but the pixels;
 * no host synchronisation.  _emit (same sizes, camera and workspace, untouched in between; n_pairs as counted, below 2^31; lists: device int32 [n_pairs]
 * of scratch, sized by the counted total and by nothing else) writes face, depth, bary and counts[O2345_RASTER_PIXELS].  _shade writes kind, rgb, nrm.
 * Integer atomics appear in the binning only, none on pixels; no kernel waits for another workgroup; the same bytes on every run.
 * Limits: no near clipping (a face with a corner in front of `near` is dropped whole), one sample per pixel (no anti-aliasing), corners snapped to 1/256
 * pixel, a face with a corner beyond 2^21 pixels is dropped.  Texture-atlas sampling is o2345_mesh_raster_shade_textured's, below: it starts from face +
 * bary. */
enum { O2345_RASTER_BAD_INDEX = 0, O2345_RASTER_NONFINITE = 1, O2345_RASTER_NEAR = 2, O2345_RASTER_RANGE = 3, O2345_RASTER_DEGENERATE = 4,
       O2345_RASTER_CULLED = 5, O2345_RASTER_OFFSCREEN = 6, O2345_RASTER_BINNED = 7, O2345_RASTER_PAIRS = 8, O2345_RASTER_PIXELS = 9,
       O2345_RASTER_COUNTS = 10 };
size_t o2345_mesh_raster_workspace_bytes(long long nv, long long nt, int H, int W);
int o2345_mesh_raster_count(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, const float* K_host,
                            const float* c2w_host, int H, int W, double near, int cull, void* workspace, size_t workspace_bytes, long long* counts, void* stream);
int o2345_mesh_raster_emit(long long nv, long long nt, const float* K_host, const float* c2w_host, int H, int W, double near, int cull, int ray_depth,
                           void* workspace, size_t workspace_bytes, long long n_pairs, int* lists, int* face, float* depth, float* bary, long long* counts,
                           void* stream);
int o2345_mesh_raster_shade(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, const int* face, const float* bary, int H, int W,
                            const float* colors_or_null, const float* normals_or_null, uint8_t* kind, float* rgb, float* nrm, void* stream);
/* Textured shading (additive since 2.3; none in the reference): a second shading stage behind the same visibility, on the buffers a textured asset file
 * holds, in the asset's own frame.  Equal to raster.shade_textured to the last bit (csrc/mesh_raster_tex_math.h is the one spelling): fp64, one operation
 * at a time, in the order written; a dot product is (x x + y y) + z z; every result is rounded to float32 once.  Inputs, device, only read: the soup
 * verts fp64 [nv,3] and tris [nt,3] (a file: its positions widened, tris = 0, 1, 2, ...), face int32 [H W] and bary float32 [H W,3] of _emit, uv float32
 * [nt,3,2] per stored corner (the file's TEXCOORD_0), image uint8 [tex_h,tex_w,4] (4-byte aligned; a side <= 16384, tex_h tex_w < 2^31), and all three or
 * none of normal_image uint8 [tex_h,tex_w,4], normals float32 [3 nt,3], tangents float32 [3 nt,4] (the file's NORMAL / TANGENT; the frame of triangle t is
 * read at corner 3t).  The camera as for the other raster entries; ambient in [0, 1].  Per pixel whose face is in [0, nt) and has its three indices in
 * [0, nv) (any other pixel is a miss: kind 0, everything 0):
 *   uv        u = (b0 u0 + b1 u1) + b2 u2, v likewise, bary widened.  u or v not finite: rgb 0, lit 0, nrm the flat normal (N of corner 3t with a normal
 *             map), counted (bad_uv); the pixel is still a hit.
 *   fetch     mesh_io.sample_texture: x = u Wt - 0.5, y = v Ht - 0.5, x0 = floor(x), fx = x - x0, y0 and fy likewise; taps (0,0), (1,0), (0,1), (1,1) at
 *             column clamp(x0 + dx, 0, Wt - 1), row clamp(y0 + dy, 0, Ht - 1): the sum and the clamp are done in floating point, the conversion to an
 *             integer comes last, so that no uv overflows an index; weights (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy; value = ((w00 c00 + w10
 *             c10) + w01 c01) + w11 c11 per channel on the bytes widened.  Albedo rgb = float32(value / 255.0), channels 0 - 2.
 *   normal    without a normal map: the unnormalised flat (P1 - P0) x (P2 - P0) of the fp64 vertices, as _shade gives it.  With one: s = the same fetch of
 *             the normal image, (x, y, z) = s / 255.0 * 2.0 - 1.0; N, T, w of corner 3t promoted; B = w (N x T); m = (x T + y B) + z N; l = sqrt(m . m);
 *             nrm = float32(m / l).  A triangle with mesh_texture_frames' degenerate mark (TANGENT.y is a negative zero), or an l that is zero or not
 *             finite: nrm = N, counted (flat_frame).
 *   lit       d_k = (R_k0 vx + R_k1 vy) + R_k2 with v as in the depth, divided by sqrt(d . d): the pixel's ray in the mesh's frame; n = nrm widened,
 *             divided by sqrt(n . n), or 0 if that length is zero or not finite; c = n . d; s = -c if -c > 0, else 0; lit = float32(rgb (ambient + (1 -
 *             ambient) s)) per channel, rgb the float32 albedo widened.  c > 0 is counted (back_lit, informative).  Both vectors live in the mesh's
 *             frame: the term does not depend on the handedness of the camera matrix, whose 3 x 3 may be a reflection (|R^T R - I| is all that is tested).
 * Outputs, device: kind uint8 [H W], rgb, nrm, lit float32 [H W,3]; counters int64 [4], 8-byte aligned = {bad_uv, flat_frame, back_lit, reserved}, zeroed
 * and written by this call, read by the caller with its own copy.  Refused: bad sizes, an atlas over 16384 on a side or with tex_h tex_w >= 2^31, a normal
 * image without frames or frames without one, ambient outside [0, 1] or not finite, the camera refusals of the other entries.  One lane per pixel, four
 * (eight) 4-byte texel loads, no LDS, one ballot and at most one atomic per counter and wave; no host synchronisation.
 * Limits: one bilinear sample per pixel, no mip maps, CLAMP_TO_EDGE only, a Lambert headlight and nothing else. */
int o2345_mesh_raster_shade_textured(const double* verts, const void* tris, int index_bytes, long long nv, long long nt, const int* face, const float* bary,
                                     const float* uv, const uint8_t* image, int tex_h, int tex_w, const uint8_t* normal_image_or_null,
                                     const float* normals_or_null, const float* tangents_or_null, const float* K_host, const float* c2w_host, int H, int W,
                                     float ambient, uint8_t* kind, float* rgb, float* nrm, float* lit, long long* counters, void* stream);
/* ---- ray cast against a mesh, and ambient occlusion (additive since 2.3.1; none in the reference: its meshes carry vertex colours only and are lit
 * in another program) ----
 * Read-only; equal to the host twins mesh_io.ray_cast and mesh_io.mesh_occlusion to the last bit, through a grid or without one.  Everything is fp64, one
 * operation at a time, in the order written (csrc/mesh_raycast_math.h and csrc/mesh_intersect_math.h are the text); a dot product is (x x + y y) + z z;
 * only comparisons decide.  verts device fp64 [nv,3], tris device int32 / int64 [nt,3] (index_bytes 4 / 8), both only read; 0 <= nv < 2^30, 3 * nt < 2^31;
 * nt = 0 is legal (nothing is hit).  n < 2^28.
 *   usable     a triangle takes part iff its indices lie in [0, nv), its nine coordinates are finite and n . n != 0 for n = (P1 - P0) x (P2 - P0).
 *   hit        the segment P -> Q hits the triangle (A, B, C), corners in stored order, iff the "crossing" of the self-intersection entries above holds:
 *              sP = orient(A,B,C,P) and sQ = orient(A,B,C,Q) strictly of opposite sign, and orient(P,Q,A,B), orient(P,Q,B,C), orient(P,Q,C,A) all > 0 or
 *              all < 0.  A zero or a NaN anywhere: no hit.  A segment with a non-finite coordinate hits nothing.  t = sP / (sP - sQ).
 *   nearest    the smallest t over the usable triangles that are hit, among equal t the smallest triangle index; a NaN t (overflowing determinants) never
 *              wins.  (inf, -1) without a hit.
 *   frame      of a direction n: len = sqrt((n_x n_x + n_y n_y) + n_z n_z); zero or not finite: no frame.  N = n / len per component; s = copysign(1, N_z);
 *              a = -1 / (s + N_z); b = (N_x N_y) a; T = (1 + (s N_x)(N_x a), s b, -(s N_x)); B = (b, s + (N_y N_y) a, -N_y).
 *   occlusion  of point p: n is dirs[i]; or, with owners, the face normal (P1 - P0) x (P2 - P0) of triangle owners[i], multiplied by -1 when dirs is given
 *              too and its dot product with dirs[i] is < 0 (a zero or NaN direction turns nothing).  An owner outside [0, nt) or not usable, or a direction
 *              without a frame, casts nothing and is counted.  P = p + bias N; Q_i = P + max_distance d_i with d_i = (x_i T + y_i B) + z_i N per
 *              component, (x_i, y_i, z_i) row i of table (device fp64 [n_samples,3], 1 <= n_samples <= 1024: mesh_io.occlusion_directions; no sine is
 *              evaluated on the device).  hits[i] = the number of i with any hit, int32 and exact.
 * o2345_mesh_ray_cast: p, q device fp64 [n,3].  any_hit == 0: t device fp64 [n], tri device int32 [n] = the nearest hit.  any_hit != 0: tri[i] = 1 / 0,
 * t is not touched and may be NULL.
 * o2345_mesh_occlusion: points device fp64 [n,3]; dirs_or_null device fp64 [n,3]; owners_or_null device int32 [n]; one of the two at least.  max_distance
 * finite and > 0, bias finite and >= 0.  hits device int32 [n]; counters device int64 [4], 8-byte aligned = {points with a non-finite coordinate, other
 * points without a frame (direction or owner), rays cast, reserved}, zeroed and written by this call.  Points of the first two kinds have hits 0.
 * grid: the grid object of o2345_mesh_distance_grid_emit over the same verts and tris, with its size and the max_cells it was built with: the segment is
 * walked slab by slab along its dominant axis, each slab visiting the cells its part of the segment can touch, widened by 2^-30 of the coordinates; the
 * nearest-hit walk stops at the first slab entered behind the best t, the any-hit walk at its first hit.  grid NULL: every triangle, for nt <= 2^16.  The
 * same bytes either way and whatever the cell edge.  A segment outside the grid's box is legal.  No workspace, no host synchronisation; one lane per
 * segment, or per (point, direction) with one ballot and one integer atomicAdd per point-row of a wave; no floating-point atomics.
 * Limits: a segment through a shared edge or vertex of two triangles hits neither (rays leak there); the unfiltered fp64 determinants may take the wrong
 * sign next to a degeneracy, and the t of a grazing hit is as inexact as they are (the twin computes the same one); binary visibility, no distance
 * falloff; no all-hits list (hit parity needs de-duplicated hits). */
int o2345_mesh_ray_cast(const double* p, const double* q, long long n, const double* verts, const void* tris, int index_bytes, long long nv, long long nt,
                        const void* grid, size_t grid_bytes, long long max_cells, int any_hit, double* t, int* tri, void* stream);
int o2345_mesh_occlusion(const double* points, const double* dirs_or_null, const int* owners_or_null, long long n, const double* table, int n_samples,
                         double max_distance, double bias, const double* verts, const void* tris, int index_bytes, long long nv, long long nt, const void* grid,
                         size_t grid_bytes, long long max_cells, int* hits, long long* counters, void* stream);
/* Load every code object of the library on the current device now (the HIP runtime loads a translation unit's kernels at its first launch: 5 - 60 ms
 * each for the units of this library, which otherwise land inside the first calls of a fresh process).  Launches nothing that touches user memory. */
int o2345_preload(void);

#ifdef __cplusplus
}
#endif
#endif
