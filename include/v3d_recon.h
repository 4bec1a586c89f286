/* v3d_recon.h - C ABI of libv3d_recon.so (v3d_amd/csrc_recon/geom.hip): geometry from the reconstructed splats.  Forward only; its own
 * library, beside libv3d_hip.so whose rasterizer intermediates it consumes (include/v3d_hip.h "Gaussian-splat reconstruction").
 *   per view:  v3d_recon_depth_alpha (expected depth + accumulated alpha of every pixel)  ->  v3d_recon_tsdf_integrate (one view into the volume)
 *   once:      v3d_recon_cells_flag -> scan -> v3d_recon_cells_vertices;  v3d_recon_edges_flag -> scan -> v3d_recon_edges_faces
 * (naive surface nets: one vertex per sign-changing cell, one quad per sign-changing grid edge; no marching-cubes tables).  The scans are
 * v3d_gs_scan of libv3d_hip.so, called by the host between the passes.
 * The volume is a cube of N^3 voxels (2 <= N <= 512: voxel, cell and edge indices are int32), axis-aligned, centred at the origin, half-extent
 * `bound`; voxel (ix, iy, iz) has linear index (iz N + iy) N + ix and centre -bound + (i + 0.5) 2 bound / N on every axis.  A cell is the cube
 * between 8 neighbouring voxel CENTRES: cell (cx, cy, cz), 0 <= c < N - 1, has linear index (cz (N-1) + cy) (N-1) + cx and corner voxels c + {0,1}.
 * Grid edge (axis a, voxel v) joins voxel v and its +1 neighbour on axis a; linear index a N^3 + v.
 * No atomics anywhere: every output is bit-reproducible.  All array pointers are device pointers, fp32 / int32, contiguous; the camera is a
 * HOST pointer.  Every entry validates its arguments before any launch: 0, or -1 (argument) / -2 (launch) with a message in
 * v3d_recon_last_error(). */
#ifndef V3D_RECON_H
#define V3D_RECON_H
#include <stdint.h>

#include "v3d_hip.h" /* v3d_gs_camera, v3d_stream_t */
#ifdef __cplusplus
extern "C" {
#endif

#define V3D_RECON_ABI_VERSION 1
#define V3D_RECON_MAX_N 512

int v3d_recon_abi_version(void);
const char* v3d_recon_last_error(void);

/* One 256-thread block per 16 x 16 tile, 256 Gaussians per LDS batch (the launch shape of v3d_gs_render_fwd).  Every pixel walks its tile's
 * sorted list with the alpha rule of the colour pass (power <= 0, alpha = min(0.99, opacity exp(power)), skipped below 1/255) and stops after
 * its own n_contrib entries, the last contributor of the colour image:  out_depth [H][W] = sum alpha_i T_i z_i  (NOT divided by alpha, as the
 * published rasterizer returns it),  out_alpha [H][W] = 1 - T.  ranges, vals_sorted, means2d, conic_opacity, depth (view z per Gaussian),
 * n_contrib: outputs of the v3d_gs_* forward of the same view.  vals_sorted may be NULL when every range is empty. */
int v3d_recon_depth_alpha(const int32_t* ranges, const uint32_t* vals_sorted, const float* means2d, const float* conic_opacity, const float* depth,
                          const int32_t* n_contrib, int32_t width, int32_t height, float* out_depth, float* out_alpha, v3d_stream_t stream);

/* One view into the volume, one thread per voxel.  The voxel centre goes through cam->view (z) and cam->proj (pixel); skipped when
 * z <= 0.2 or the nearest pixel lies outside the image.  alpha_map < alpha_min there: seen empty, tsdf_sum += 1, weight += 1 (the visual-hull
 * carve).  Otherwise sdf = depth_map / alpha_map - z: skipped below -trunc; else tsdf_sum += min(1, sdf / trunc), weight += 1 and, when
 * |sdf| <= trunc, rgb_sum += the pixel's colour, rgb_weight += 1.  image [3][H][W]; tsdf_sum, weight, rgb_weight [N^3]; rgb_sum [3][N^3]. */
int v3d_recon_tsdf_integrate(const float* depth_map, const float* alpha_map, const float* image, const v3d_gs_camera* cam, int32_t N, float bound,
                             float trunc, float alpha_min, float* tsdf_sum, float* weight, float* rgb_sum, float* rgb_weight, v3d_stream_t stream);

/* flags [(N-1)^3] = 1 where all 8 corners have weight > 0 and their mean TSDF (tsdf_sum / weight; negative = inside) changes sign, else 0 */
int v3d_recon_cells_flag(const float* tsdf_sum, const float* weight, int32_t N, int32_t* flags, v3d_stream_t stream);
/* One vertex per flagged cell at row offsets[cell] (exclusive scan of flags): the mean of the linearly interpolated zero crossings of the
 * cell's sign-changing edges; colour = mean of rgb_sum / rgb_weight over the corners with rgb_weight > 0 (0.5 grey when none has).
 * verts, colors [n_active][3]. */
int v3d_recon_cells_vertices(const float* tsdf_sum, const float* weight, const float* rgb_sum, const float* rgb_weight, int32_t N, float bound,
                             const int32_t* flags, const int32_t* offsets, float* verts, float* colors, v3d_stream_t stream);
/* flags [3 N^3] = 1 for every grid edge whose two voxels differ in sign and whose 4 adjacent cells exist and are flagged, else 0 */
int v3d_recon_edges_flag(const float* tsdf_sum, const float* weight, int32_t N, const int32_t* cell_flags, int32_t* flags, v3d_stream_t stream);
/* Two triangles per flagged edge at rows 2 edge_offsets[edge], + 1 (exclusive scan of the edge flags), joining the 4 adjacent cells' vertices
 * (cell_offsets), wound so that the normal points from the negative to the positive voxel.  faces [2 n_edges][3]. */
int v3d_recon_edges_faces(const float* tsdf_sum, const float* weight, int32_t N, const int32_t* cell_offsets, const int32_t* edge_flags,
                          const int32_t* edge_offsets, int32_t* faces, v3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
