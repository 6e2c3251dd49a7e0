// Error reporting + version for the o2345 C-ABI (see include/o2345.h).
#include <stdarg.h>
#include <stdio.h>
#include "common.h"

namespace o2345 {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
}  // namespace o2345

#include <stddef.h>

namespace o2345 {
int preload_costvol();
int preload_sparse();
int preload_sparse_mfma();
int preload_sdf_mlp();
int preload_sdf_mlp_x3();
int preload_render();
int preload_list_sort();
int preload_color_maps();
int preload_color_pts();
int preload_mcubes();
int preload_mesh_components();
int preload_mesh_smooth();
int preload_mesh_decimate();
int preload_mesh_simplify();
int preload_mesh_project();
int preload_mesh_pack();
int preload_mesh_export();
int preload_mesh_texture();
int preload_mesh_distance();
int preload_mesh_align();
int preload_mesh_audit();
int preload_mesh_fill();
int preload_mesh_intersect();
int preload_mesh_raster();
int preload_mesh_raycast();
int preload_surface_trace();
int preload_featmaps();
int preload_convnet();
}

extern "C" {
const char* o2345_last_error(void) { return o2345::g_err; }
int o2345_version(void) { return 231; }     // 2.3.1: the raster entries take the camera as K_host, c2w_host; 2.3: O2345SimplifyStats, O2345AuditStats; 2.2: declared stats structs, o2345_struct_size / _layout; 2.1: segment_rays + weight_cull in O2345RenderIO; 2.0: see include/o2345.h (1.5: o2345_list_sort_by_visibility; 1.4: color stats, bf16 entry removed; 1.3: o2345_conv2d family; 1.2: t_rand)

int o2345_preload(void) {
    int e, bad = 0;
    if ((e = o2345::preload_costvol())) bad = e;
    if ((e = o2345::preload_sparse())) bad = e;
    if ((e = o2345::preload_sparse_mfma())) bad = e;
    if ((e = o2345::preload_sdf_mlp())) bad = e;
    if ((e = o2345::preload_sdf_mlp_x3())) bad = e;
    if ((e = o2345::preload_render())) bad = e;
    if ((e = o2345::preload_list_sort())) bad = e;
    if ((e = o2345::preload_color_maps())) bad = e;
    if ((e = o2345::preload_color_pts())) bad = e;
    if ((e = o2345::preload_mcubes())) bad = e;
    if ((e = o2345::preload_mesh_components())) bad = e;
    if ((e = o2345::preload_mesh_smooth())) bad = e;
    if ((e = o2345::preload_mesh_decimate())) bad = e;
    if ((e = o2345::preload_mesh_simplify())) bad = e;
    if ((e = o2345::preload_mesh_project())) bad = e;
    if ((e = o2345::preload_mesh_pack())) bad = e;
    if ((e = o2345::preload_mesh_export())) bad = e;
    if ((e = o2345::preload_mesh_texture())) bad = e;
    if ((e = o2345::preload_mesh_distance())) bad = e;
    if ((e = o2345::preload_mesh_align())) bad = e;
    if ((e = o2345::preload_mesh_audit())) bad = e;
    if ((e = o2345::preload_mesh_fill())) bad = e;
    if ((e = o2345::preload_mesh_intersect())) bad = e;
    if ((e = o2345::preload_mesh_raster())) bad = e;
    if ((e = o2345::preload_mesh_raycast())) bad = e;
    if ((e = o2345::preload_surface_trace())) bad = e;
    if ((e = o2345::preload_featmaps())) bad = e;
    if ((e = o2345::preload_convnet())) bad = e;
    O2345_REQUIRE(bad == 0, "preload: hipFuncGetAttributes failed (%s)", hipGetErrorString((hipError_t)bad));
    return 0;
}

const char* o2345_knobs(void) {
    static const struct Text { char s[160]; Text() { const o2345::Knobs& k = o2345::knobs();
        snprintf(s, sizeof s, "list_sort=%d sparse_brick=%d flat_sched=%d color_tiles=%d color_sched=%d ray_stream_min=%lld tile_queue=%d", k.list_sort, k.sparse_brick,
                 k.flat_sched, k.color_tiles, k.color_sched, k.ray_stream_min, k.tile_queue); } } t;
    return t.s;
}

// layout of every struct include/o2345.h declares, as compiled into this library: fields in declaration order, structs in the header's order; the ctypes
// binding compares the structs it generated from the header's text with this
#define F(name) offsetof(S, name)
#define S O2345RenderIO
static const size_t off_render_io[] = {
    F(sdf_blob), F(color_x3_blob), F(color_mfma_blob), F(vol_cl), F(maskvol), F(cmaps), F(proj), F(cam_pos), F(D), F(V), F(H), F(W),
    F(rays_o), F(rays_d), F(near_ray), F(far_ray), F(query_cam), F(t_rand), F(R), F(n_samples), F(n_importance), F(sdf_mode), F(segment_rays),
    F(near), F(far), F(sample_dist), F(inv_s), F(alpha_inter_ratio), F(background), F(weight_cull),
    F(mid_z), F(dists), F(pm), F(sdf), F(grad), F(rgb), F(nviews), F(color), F(depth), F(weights), F(cdf), F(weights_sum), F(weights_max),
    F(depth_var), F(alpha_sum), F(grad_err), F(color_mask), F(z_vals), F(scalars), F(color_stats)};
#undef S
#define S O2345ProjectStats
static const size_t off_project[] = {F(n_nonfinite), F(converged), F(unconverged), F(stalled), F(clamped), F(max_before), F(max_after), F(reserved), F(count)};
#undef S
#define S O2345TextureStats
static const size_t off_texture[] = {F(n_nonfinite), F(n_bad)};
#undef S
#define S O2345SurfaceStats
static const size_t off_surface[] = {F(hits), F(entry_hits), F(box_misses), F(misses), F(stalled), F(bad_rays), F(samples), F(lookups), F(n_list), F(reserved)};
#undef S
#define S O2345DistanceStats
static const size_t off_distance[] = {F(sum_w), F(sum_wd), F(sum_wd2), F(within), F(max_d2_bits), F(n), F(n_unmatched), F(n_degenerate), F(n_bad)};
#undef S
#define S O2345SimplifyStats
static const size_t off_simplify[] = {F(rounds), F(vertices), F(triangles), F(stopped), F(max_cost_bits), F(reserved)};
#undef S
#define S O2345AuditStats
static const size_t off_audit[] = {
    F(bad_index), F(nonfinite), F(vertices), F(edges), F(faces), F(repeated_faces), F(zero_area_faces), F(boundary_edges), F(nonmanifold_edges),
    F(inconsistent_edges), F(creased_edges), F(boundary_vertices), F(nonmanifold_vertices), F(bowtie_vertices), F(unused_vertices), F(reserved), F(histogram),
    F(area), F(volume6), F(quality_sum), F(quality_min), F(edge2_min), F(edge2_max)};
#undef S
#undef F
#define LAYOUT(type, off) {sizeof(type), off, (int)(sizeof off / sizeof off[0])}
static const struct { size_t size; const size_t* off; int n; } layouts[] = {
    LAYOUT(O2345RenderIO, off_render_io), LAYOUT(O2345ProjectStats, off_project), LAYOUT(O2345TextureStats, off_texture),
    LAYOUT(O2345SurfaceStats, off_surface), LAYOUT(O2345DistanceStats, off_distance), LAYOUT(O2345SimplifyStats, off_simplify),
    LAYOUT(O2345AuditStats, off_audit)};
#undef LAYOUT
static const int n_layouts = (int)(sizeof layouts / sizeof layouts[0]);

size_t o2345_struct_size(int which) { return which >= 0 && which < n_layouts ? layouts[which].size : 0; }
int o2345_struct_layout(int which, size_t* offsets_host, int n) {
    if (which < 0 || which >= n_layouts) return 0;
    for (int i = 0; i < n && i < layouts[which].n && offsets_host; ++i) offsets_host[i] = layouts[which].off[i];
    return layouts[which].n;
}
}
