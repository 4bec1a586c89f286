/* v3d_recon.h - C ABI of libv3d_recon.so (v3d_amd/csrc_recon/): geometry from the reconstructed splats and the refinement of the mesh's colours.  Its own
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

/* ---- Mesh rasterizer (v3d_amd/csrc_recon/meshrast.hip; host side: v3d_amd/recon/mesh_render.py) ------------------------------------------
 * Renders the extracted triangle mesh from one camera.  Forward only, no atomics, bit-reproducible.  Per view:
 *   v3d_recon_mesh_project -> v3d_recon_mesh_face_setup -> scan of tiles_touched -> v3d_recon_mesh_duplicate_keys -> sort of the pairs on
 *   32 + bits(tiles) key bits -> v3d_recon_mesh_tile_ranges -> v3d_recon_mesh_render
 * (the binning of the splat rasterizer; the scan and the sort are v3d_gs_scan and v3d_gs_radix_sort_pairs of libv3d_hip.so, called by the
 * host, which reads the scan's total back and refuses one above INT32_MAX).
 * Pixel (i, j) has its centre at coordinate (i, j) (the convention of the splat rasterizer's ndc2Pix).  Vertices are snapped to a grid of
 * 2^subpixel_bits steps per pixel (0 .. 8 bits); coverage is decided on those integers alone, with int64 edge functions.  Images are at most
 * 4096 pixels on a side.
 * Marked vertices: view z <= 0.2, a position that is not finite, or one beyond 2^28 sub-pixel steps from the origin (the edge functions must
 * stay inside int64).  A face that uses a marked vertex is not drawn: THERE IS NO NEAR-PLANE CLIPPING, a face with a corner at z <= 0.2 is
 * dropped whole.  The orbit cameras sit at radius 2 around a volume of half-extent about 1.1, so on the documented path no vertex comes
 * nearer than 0.4 and this never happens.
 * Front faces: view axes are x right, y down, z forward, and pixels run the same way, so a face whose corners run counter-clockwise seen from
 * outside (outward normal, the winding v3d_recon_edges_faces writes) and which looks at the camera has a NEGATIVE doubled area
 * (b - a) x (c - a) of its snapped corners.  cull = 1 drops the faces of positive area. */
#define V3D_RECON_MESH_MAX_IMAGE 4096
#define V3D_RECON_MESH_MAX_SUBPIXEL_BITS 8

/* One thread per vertex, verts [V][3].  View z through cam->view and the pixel position through cam->proj, the statements of the TSDF pass:
 * px = ((hx / (hw + 1e-7) + 1) W - 1) / 2, py likewise with H.  zv [V]; pix_f [V][2] (fp32 pixel position); pix_q [V][2] (int32: px, py times
 * 2^subpixel_bits, rounded to nearest, ties to even; both INT32_MIN on a marked vertex). */
int v3d_recon_mesh_project(const float* verts, int32_t num_verts, const v3d_gs_camera* cam, int32_t subpixel_bits, float* zv, float* pix_f,
                           int32_t* pix_q, v3d_stream_t stream);

/* One thread per face, faces [F][3] (a face with an index outside 0 .. V-1 is not drawn).  A face is drawn when none of its vertices is
 * marked, its doubled area (int64, of the snapped corners) is not 0, it is a front face or cull = 0, and the bounding box of the pixel centres
 * it can cover, clamped to the image, is not empty.  tiles_touched [F]: 16 x 16 tiles under that box, 0 for a face that is not drawn;
 * zmin [F]: the smallest view z of the three vertices. */
int v3d_recon_mesh_face_setup(const int32_t* faces, int32_t num_faces, const int32_t* pix_q, const float* zv, int32_t num_verts, int32_t width,
                              int32_t height, int32_t subpixel_bits, int32_t cull, int32_t* tiles_touched, float* zmin, v3d_stream_t stream);

/* keys [n] = tile << 32 | float bits of zmin, vals [n] = face, row-major over the face's tile rectangle, at rows offsets[face] .. (offsets:
 * exclusive scan of tiles_touched, n its total). */
int v3d_recon_mesh_duplicate_keys(const int32_t* faces, int32_t num_faces, const int32_t* pix_q, int32_t num_verts, const int32_t* tiles_touched,
                                  const int32_t* offsets, const float* zmin, int32_t width, int32_t height, int32_t subpixel_bits, uint64_t* keys,
                                  uint32_t* vals, v3d_stream_t stream);

/* ranges [tiles][2] = [start, end) of every tile in the sorted list, 0 0 for a tile without faces.  num_instances may be 0 (keys_sorted NULL). */
int v3d_recon_mesh_tile_ranges(const uint64_t* keys_sorted, int32_t num_instances, int32_t width, int32_t height, int32_t* ranges,
                               v3d_stream_t stream);

/* One 256-thread block per tile, one pixel per thread, 256 faces per LDS batch.  Coverage: the three int64 edge functions at the pixel centre,
 * with a top-left fill rule where one is 0, applied after orienting the face, so it holds for either winding: two faces that share an edge
 * cover every pixel centre on it exactly once.  Depth is perspective-correct: b_i = E_i / (E_0 + E_1 + E_2), z = 1 / sum(b_i / zv_i), kept
 * inside the face's own [zmin, zmax].  The nearest z wins; on bit-equal z the lower face index wins.  The winner is shaded once:
 * c = z sum(b_i c_i / zv_i) from colors [V][3].
 * image [3][H][W] (cam->bg where nothing covers), depth [H][W] (view z, 0 where nothing covers), alpha [H][W] (0 or 1), face_id [H][W]
 * (-1 where nothing covers), n_hit [H][W] (number of drawn faces that cover the pixel centre) or NULL.
 * The lists are ordered by zmin.  With n_hit NULL a block leaves its list before the first batch whose first zmin lies behind the depth every
 * one of its pixels already holds (strictly: at equal depth a later face of lower index would still win); with n_hit every list is walked to
 * its end.  With cull = 0 a closed mesh gives an even n_hit on every pixel.  vals_sorted may be NULL when every range is empty. */
int v3d_recon_mesh_render(const int32_t* ranges, const uint32_t* vals_sorted, const int32_t* faces, int32_t num_faces, const int32_t* pix_q,
                          const float* zv, const float* zmin, const float* colors, const v3d_gs_camera* cam, int32_t subpixel_bits, float* image,
                          float* depth, float* alpha, int32_t* face_id, int32_t* n_hit, v3d_stream_t stream);

/* ---- Mesh colour refinement (v3d_amd/csrc_recon/meshshade.hip; host side: v3d_amd/recon/mesh_refine.py) -----------------------------------
 * Optimises the vertex colours of the mesh against images of known cameras with the geometry held fixed.  What a camera sees then never
 * changes, so the rasterizer above runs ONCE per view and its result is frozen: the image is a fixed sparse linear map of the colours (three
 * coefficients per covered pixel, the background elsewhere) and the gradient with respect to the colours is the transpose of that map.
 *   per view, once:  v3d_recon_mesh_render -> v3d_recon_mesh_pixel_weights -> scan of the coverage -> v3d_recon_mesh_vertex_records -> sort of
 *                    the records on max(1, bits(V - 1)) key bits -> v3d_recon_mesh_vertex_ranges;  the host then gathers
 *                    ent_pix [n] = value / 3 and ent_w [n] = depth[pixel] pix_w[value] from the sorted values
 *   per iteration:   v3d_recon_mesh_shade -> (loss on the host side) -> v3d_recon_mesh_shade_bwd -> v3d_recon_mesh_color_adam
 * (the scan and the sort are v3d_gs_scan and v3d_gs_radix_sort_pairs of libv3d_hip.so, called by the host).  No atomics: the sort is stable,
 * so a vertex's entries stay in ascending pixel order, and one wave sums them in an order that the list alone decides.  There is no gradient
 * through coverage (no silhouette antialiasing): vertex positions are not parameters. */

/* One thread per pixel, on the face_id map of v3d_recon_mesh_render and the pix_q, zv of the same view.  pix_vert [H][W][3]: the three vertex
 * indices of the winning face, -1 -1 -1 where face_id < 0;  pix_w [H][W][3]: b_k / zv[i_k] with b_k from the int64 edge functions, the
 * orientation flip and the fp32 quotients of the render kernel, statement for statement; 0 where nothing covers. */
int v3d_recon_mesh_pixel_weights(const int32_t* face_id, const int32_t* faces, int32_t num_faces, const int32_t* pix_q, const float* zv,
                                 int32_t num_verts, int32_t width, int32_t height, int32_t subpixel_bits, int32_t* pix_vert, float* pix_w,
                                 v3d_stream_t stream);

/* One thread per pixel: image [3][H][W], image[ch][p] = depth[p] (w_0 c[i_0][ch] + w_1 c[i_1][ch] + w_2 c[i_2][ch]) from colors [V][3], the
 * statement the render kernel shades with; bg0 bg1 bg2 where pix_vert is -1.  depth [H][W]: the render's view z. */
int v3d_recon_mesh_shade(const int32_t* pix_vert, const float* pix_w, const float* depth, const float* colors, int32_t num_verts, int32_t width,
                         int32_t height, float bg0, float bg1, float bg2, float* image, v3d_stream_t stream);

/* One thread per pixel: three records per covered pixel at rows 3 offsets[pixel] .. + 2 (offsets: exclusive scan of pix_vert[pixel][0] >= 0,
 * num_records = 3 x its total, positive), keys = vertex index, vals = 3 pixel + k: in pixel order. */
int v3d_recon_mesh_vertex_records(const int32_t* pix_vert, const int32_t* offsets, int32_t width, int32_t height, int32_t num_records, uint64_t* keys,
                                  uint32_t* vals, v3d_stream_t stream);

/* ranges [V][2] = [start, end) of every vertex in the sorted records, 0 0 for a vertex without one.  num_records may be 0 (keys_sorted NULL). */
int v3d_recon_mesh_vertex_ranges(const uint64_t* keys_sorted, int32_t num_records, int32_t num_verts, int32_t* ranges, v3d_stream_t stream);

/* The transpose of the shade: dL_dcolors [V][3] from dL_dimage [3][H][W], dL_dcolors[v][ch] = sum over the entries e of vertex v of
 * ent_w[e] dL_dimage[ch][ent_pix[e]].  One 64-lane wave per vertex: lane l adds entries start + l, start + l + 64, .. in list order, the
 * lanes then meet in an xor butterfly, so the result does not depend on the launch shape.  Every row is written, 0 0 0 for a vertex without
 * entries: the caller need not clear the buffer.  A gradient on an uncovered pixel reaches no vertex.  num_entries may be 0 (ent_pix, ent_w NULL). */
int v3d_recon_mesh_shade_bwd(const int32_t* ranges, const int32_t* ent_pix, const float* ent_w, int32_t num_entries, const float* dL_dimage,
                             int32_t width, int32_t height, int32_t num_verts, float* dL_dcolors, v3d_stream_t stream);

/* One thread per element of [V][3], in place on logit, m, v.  grad is dL/dcolors with colors = sigmoid of logit: g = grad s (1 - s), then the
 * update of torch.optim.Adam (m lerped towards g by 1 - beta1, v = beta2 v + (1 - beta2) g g, bias corrections of `step` = 1, 2, .., eps added
 * outside the square root, no weight decay), then colors = sigmoid of the new logit.  An element whose grad was 0 on every step so far keeps
 * its logit bit for bit. */
int v3d_recon_mesh_color_adam(float* logit, float* m, float* v, const float* grad, int32_t num_verts, double lr, double beta1, double beta2,
                              double eps, int32_t step, float* colors, v3d_stream_t stream);

/* ---- Mesh topology (v3d_amd/csrc_recon/meshtopo.hip; host side: v3d_amd/recon/mesh_clean.py) ------------------------------------------------
 * The mesh as a graph: connected components (to drop floaters and vertices that no face uses), Taubin smoothing, vertex normals.  All of it
 * walks one structure, the list of corners that touch every vertex:
 *   once:  v3d_recon_mesh_corner_records -> sort of the records on max(1, bits(V - 1)) key bits -> v3d_recon_mesh_vertex_ranges on the sorted
 *          keys;  ranges [V][2] and corners [3F] = the sorted values.  Corner c = 3 f + k is place k of face f.  The sort is stable, so a
 *          vertex's corners ascend: that order is the summation order of everything below.
 *   normals:     v3d_recon_mesh_vertex_normals
 *   components:  labels = 0 .. V-1, then v3d_recon_mesh_label_round between two buffers until a round changes nothing
 *   filter:      v3d_recon_mesh_face_labels -> sort on max(1, bits(V)) key bits -> v3d_recon_mesh_vertex_ranges (faces per root) -> the host
 *                decides which roots stay -> v3d_recon_mesh_keep_flags -> scans of both flag arrays -> v3d_recon_mesh_compact_faces
 *   smoothing:   v3d_recon_mesh_boundary_flags (optional pins), then v3d_recon_mesh_smooth_pass between two buffers
 * (the scans and the sorts are v3d_gs_scan and v3d_gs_radix_sort_pairs of libv3d_hip.so, called by the host).  One thread per vertex (or per
 * face, or per corner); no atomics; bit-reproducible.  V >= 1, F >= 1 and 3 F <= INT32_MAX everywhere: the host handles an empty mesh without
 * a launch.  A face with an index outside 0 .. V-1 is absent for every entry below, and nothing is read through such an index. */

/* One thread per corner, faces [F][3]: keys [3F] = faces[f][k], vals [3F] = 3 f + k, in corner order.  A key outside 0 .. V-1 is written as 0
 * so that it stays inside the sorted bits: the entries below skip that corner because its face is absent. */
int v3d_recon_mesh_corner_records(const int32_t* faces, int32_t num_faces, int32_t num_verts, uint64_t* keys, uint32_t* vals, v3d_stream_t stream);

/* normals [V][3]: the sum over the vertex's list, in list order, of (v1 - v0) x (v2 - v0) of the face (area weighting), divided by its length;
 * 0 0 1 where the squared length of the sum is not above 1e-20 (no face, no area, or normals that cancel).  verts [V][3]. */
int v3d_recon_mesh_vertex_normals(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                  const int32_t* corners, float* normals, v3d_stream_t stream);

/* One round of the component labelling, from labels_in [V] to labels_out [V] (two buffers):  m = min(labels_in[v], labels_in of every corner of
 * every face of v's list),  labels_out[v] = labels_in[m]  (one pointer jump).  Started from labels[v] = v, a label always names a vertex of the
 * same component with an index <= the vertex's own; the fixed point is the smallest index of the component (a vertex without faces keeps
 * itself).  Two vertices are joined when a face uses both.  A thread whose label changed stores 1 to changed [1], which the caller cleared;
 * nothing else is written there.  Plain min-propagation ends within diameter + 1 rounds and the jump only lowers labels: V + 8 rounds without
 * a fixed point mean broken lists. */
int v3d_recon_mesh_label_round(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                               const int32_t* labels_in, int32_t* labels_out, int32_t* changed, v3d_stream_t stream);

/* One thread per face: keys [F] = labels[faces[f][0]], vals [F] = f, in face order; the key V for an absent face (sort on bits(V) bits:
 * v3d_recon_mesh_vertex_ranges with V vertices then ignores it).  The ranges of the sorted keys give every root's number of faces. */
int v3d_recon_mesh_face_labels(const int32_t* faces, int32_t num_faces, const int32_t* labels, int32_t num_verts, uint64_t* keys, uint32_t* vals,
                               v3d_stream_t stream);

/* keep_root [V]: 1 at the roots (labels at their fixed point) of the components that stay.  keep_face [F] = keep_root[labels[faces[f][0]]];
 * keep_vert [V] = keep_root[labels[v]] and the vertex has at least one face. */
int v3d_recon_mesh_keep_flags(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                              const int32_t* labels, const int32_t* keep_root, int32_t* keep_face, int32_t* keep_vert, v3d_stream_t stream);

/* One thread per face: faces_out[face_off[f]][k] = vert_off[faces[f][k]] for every kept face (face_off, vert_off: exclusive scans of keep_face
 * and keep_vert; num_faces_out, num_verts_out their totals, both positive).  The order of faces and of vertices is kept. */
int v3d_recon_mesh_compact_faces(const int32_t* faces, int32_t num_faces, int32_t num_verts, const int32_t* keep_face, const int32_t* face_off,
                                 const int32_t* keep_vert, const int32_t* vert_off, int32_t num_faces_out, int32_t num_verts_out, int32_t* faces_out,
                                 v3d_stream_t stream);

/* flags [V] = 1 where the vertex lies on an open edge.  The entry of v's list at corner k has the two neighbours faces[f][(k + 1) % 3] and
 * faces[f][(k + 2) % 3]; the flag is set when some neighbour other than v is a neighbour in exactly one entry (on a closed manifold every
 * neighbour is in two).  Quadratic in the length of the list. */
int v3d_recon_mesh_boundary_flags(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                                  int32_t* flags, v3d_stream_t stream);

/* One pass from verts_in [V][3] to verts_out [V][3] (two buffers):  out = in + factor (mean - in), mean = the sum over v's list, in list
 * order, of (a + b) / 2 of the entry's two neighbours, divided by the number of entries (the umbrella operator on a closed manifold, where
 * every neighbour comes twice).  A vertex without faces is copied, and so is one with pinned[v] != 0 (pinned [V] or NULL).  Taubin smoothing
 * alternates factor = lambda > 0 and factor = mu < -lambda. */
int v3d_recon_mesh_smooth_pass(const float* verts_in, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                               const int32_t* corners, const int32_t* pinned, float factor, float* verts_out, v3d_stream_t stream);

/* ---- Mesh decimation (v3d_amd/csrc_recon/meshdecim.hip; host side: v3d_amd/recon/mesh_decimate.py) ----------------------------------------
 * Quadric-error half-edge collapse in parallel rounds.  The collapse v -> u moves v onto u: u keeps its position (and colour), the two faces on
 * the edge (v, u) die and v's other faces name u instead.  Vertices are never moved or renumbered here; a dead face holds num_verts in all
 * three places, which makes it absent for every entry of this header.
 *   once:       the corner lists (above), then v3d_recon_mesh_vertex_quadrics
 *   per round:  the corner lists of the live faces: v3d_recon_mesh_corner_records, the sort and v3d_recon_mesh_vertex_ranges called with
 *               num_verts + 1 vertices (and ranges [V + 1][2]), so that the corners of the dead faces gather on the extra vertex V, which no
 *               entry below looks at;
 *               v3d_recon_mesh_decim_propose -> v3d_recon_mesh_decim_min_round twice (keys -> min1 -> min2) -> v3d_recon_mesh_decim_accept ->
 *               sort of (sel_keys, sel_vals) on 64 bits -> v3d_recon_mesh_decim_cut -> v3d_recon_mesh_decim_apply -> scan of `live`, whose
 *               total is the next round's live_faces
 *   at the end: v3d_recon_mesh_compact_faces with keep_face = live and keep_vert = 1 - removed
 * (the scans and the sorts are v3d_gs_scan and v3d_gs_radix_sort_pairs of libv3d_hip.so, called by the host, which reads the totals and the
 * flags back once per group of rounds).  One thread per vertex (or per face); no atomics; bit-reproducible.  Positions are fp32; quadrics,
 * costs and the normal test are fp64.  V >= 1, F >= 1 and 3 F <= INT32_MAX everywhere.  The valence of a vertex is the number of its faces. */
#define V3D_RECON_MESH_MAX_VALENCE 1024

/* quadrics [V][10] (fp64): the sum over the vertex's list, in list order, of w (a b c d)^T (a b c d), upper triangle row by row (aa ab ac ad bb
 * bc bd cc cd dd), of every face with area: n = (v1 - v0) x (v2 - v0), (a b c) = n / |n|, d = -(a b c) . v0, w = |n| / 2.  Zeros without a face. */
int v3d_recon_mesh_vertex_quadrics(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                   const int32_t* corners, double* quadrics, v3d_stream_t stream);

/* One thread per vertex: keys [V], targets [V].  v is removable when it has 3 .. max_valence faces and they form one closed fan (every
 * neighbour follows v in exactly one of them and precedes it in exactly one, and walking from face to face comes round after all of them):
 * a vertex on an open edge, a non-manifold one, one without faces and one above the cap propose nothing.  v -> u for a neighbour u is valid when
 *   - the faces (v, u, a1) and (v, a2, u) on the edge have a1 != a2 and no other neighbour of v is a neighbour of u (the link condition),
 *   - u would end with at most max_valence faces (it has n_u + n_v - 4 afterwards),
 *   - every face of v without u keeps n_before . n_after > 0 for n = (v1 - v0) x (v2 - v0) before and after v is replaced by u's position
 *     (no flip, no face without area before or after),
 *   - no face of v without u would repeat the three vertices of a face u already has.
 * cost = p^T (Q_v + Q_u) p at u's position p (homogeneous), clamped at 0, rounded to fp32; a cost that is not a number is no candidate.
 * targets[v] = the valid u of the smallest fp32 cost, the smaller u among equals; keys[v] = fp32 bits of that cost << 32 | v.  Without a valid
 * neighbour keys[v] is all ones and targets[v] = -1. */
int v3d_recon_mesh_decim_propose(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                 const int32_t* corners, const double* quadrics, int32_t max_valence, uint64_t* keys, int32_t* targets,
                                 v3d_stream_t stream);

/* keys_out [V] = the smallest of keys_in over v and every corner of every face of v's list (two buffers).  Twice: the smallest key within
 * graph distance 2. */
int v3d_recon_mesh_decim_min_round(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                                   const uint64_t* keys_in, uint64_t* keys_out, v3d_stream_t stream);

/* One thread per vertex: v is a local minimum when keys[v] is not all ones and equals min2[v]; accept [V] = 1 for the local minima whose cost
 * is at most max_error (>= 0, +inf for no limit), else 0.  Keys are distinct, so two accepted vertices are at least 3 edges apart: no face
 * holds two, no two share a target, no target is accepted or next to another accepted vertex.  sel_keys [V] = keys[v] where accepted, all ones
 * elsewhere; sel_vals [V] = v.  flags [2], cleared by the caller: flags[0] = 1 when there is a local minimum, flags[1] = 1 when one is accepted
 * (the smallest key of the mesh always is a local minimum: flags[0] set with flags[1] clear means that it costs more than max_error). */
int v3d_recon_mesh_decim_accept(const uint64_t* keys, const uint64_t* min2, int32_t num_verts, float max_error, int32_t* accept, uint64_t* sel_keys,
                                uint32_t* sel_vals, int32_t* flags, v3d_stream_t stream);

/* One thread per row of the sorted (sel_keys, sel_vals): every collapse removes two faces, so only the ceil((live_faces[0] - target_faces) / 2)
 * accepted vertices of the smallest keys stay accepted (none when live_faces[0] <= target_faces); accept of the others is cleared.  live_faces
 * is a DEVICE pointer to the number of live faces. */
int v3d_recon_mesh_decim_cut(const uint64_t* sel_keys_sorted, const uint32_t* sel_vals_sorted, int32_t num_verts, const int32_t* live_faces,
                             int32_t target_faces, int32_t* accept, v3d_stream_t stream);

/* Thread t decides face t and vertex t.  faces_out [F][3] (two buffers): a face with an accepted corner v and targets[v] dies (V V V), one with
 * v alone names targets[v] in v's place, every other face is copied; an absent face becomes a dead one.  live [F] = 1 for the faces that
 * remain.  For every accepted v: quadrics[targets[v]] += quadrics[v] in place (one writer per row, and no row that is read is written) and
 * removed[v] = 1; removed is otherwise left as it is. */
int v3d_recon_mesh_decim_apply(const int32_t* faces_in, int32_t num_faces, int32_t num_verts, const int32_t* accept, const int32_t* targets,
                               int32_t* faces_out, int32_t* live, double* quadrics, int32_t* removed, v3d_stream_t stream);

/* ---- Mesh texture (v3d_amd/csrc_recon/meshtex.hip; host side: v3d_amd/recon/mesh_texture.py) ------------------------------------------------
 * A texture for the decimated mesh, fitted against images of known cameras by the method of "Mesh colour refinement" with texels in the
 * place of vertices: every view is rasterized once and frozen, the image is a gather of four texels per pixel, the gradient its transpose.
 *   once:            v3d_recon_tex_face_uvs (for the writer), v3d_recon_tex_bake_vertex_colors (the initial albedo)
 *   per view, once:  v3d_recon_mesh_render -> v3d_recon_mesh_pixel_weights -> v3d_recon_tex_pixel_texels -> scan of the coverage ->
 *                    v3d_recon_tex_texel_records -> sort of the records on max(1, bits(R R - 1)) key bits -> v3d_recon_mesh_vertex_ranges with
 *                    num_verts = R R;  the host then gathers ent_pix [n] = value / 4 and ent_w [n] = pix_tw[value] from the sorted values
 *   per iteration:   v3d_recon_tex_shade -> (loss on the host side) -> v3d_recon_tex_shade_bwd -> v3d_recon_mesh_color_adam with num_verts = R R
 * No atomics; the sort is stable, so a texel's entries stay in ascending 4 pixel + j and its thread adds them in that order.
 *
 * THE ATLAS.  The texture is R x R texels, R <= 4096, stored [R R][3] float32.  Texel (x, y) has index y R + x and its centre at coordinate
 * (x, y) (the pixel convention of the rasterizer above).  Every face owns a right triangle of texels, by integer arithmetic on its index:
 *   g = ceil(sqrt(ceil(F / 2))) cells per row;  cell size S = floor(R / g), at least 4 (a smaller one is refused: "texture too small");
 *   face f lives in cell c = f >> 1 at origin (x0, y0) = ((c % g) S, (c / g) S), in half f & 1;  with L = S - 3 the UV corners of its places
 *   0, 1, 2 are
 *     half 0:  (x0, y0)                  (x0 + L, y0)                  (x0, y0 + L)
 *     half 1:  (x0 + S-1, y0 + S-1)      (x0 + S-1 - L, y0 + S-1)      (x0 + S-1, y0 + S-1 - L)
 *   (both halves have the same orientation);  the cell's texel (i, j) is owned by half 0 when i + j <= S - 2, else by half 1;  a texel outside
 *   the g S square, or whose face index is >= F, is unowned.
 * A sample anywhere in a face's UV triangle puts all of its bilinear 2 x 2 weight on texels the face owns: nothing bleeds between faces and
 * this sampler needs no dilation.  No corner rotation and no multi-face charts: about half of the atlas is gutter. */
#define V3D_RECON_TEX_MAX_SIZE 4096
#define V3D_RECON_TEX_MIN_CELL 4

/* One thread per face: vt [F][3][2], the UV corners above in texels. */
int v3d_recon_tex_face_uvs(int32_t num_faces, int32_t tex_size, float* vt, v3d_stream_t stream);

/* One thread per texel.  owner [R R]: the face that owns the texel, -1 when unowned.  texture [R R][3]: with (i, j) the texel's place in its
 * cell, mirrored to (S-1-i, S-1-j) in half 1, b1 = clamp(i / L, 0, 1), b2 = clamp(j / L, 0, 1 - b1), b0 = 1 - b1 - b2 and the colour
 * b0 c[v0] + b1 c[v1] + b2 c[v2] from colors [V][3] and the face's vertices;  `fill` on unowned texels and on the texels of a face with an
 * index outside 0 .. V-1 (nothing is read through such an index). */
int v3d_recon_tex_bake_vertex_colors(const int32_t* faces, int32_t num_faces, const float* colors, int32_t num_verts, int32_t tex_size, float fill,
                                     int32_t* owner, float* texture, v3d_stream_t stream);

/* One thread per pixel, on the face_id map of v3d_recon_mesh_render and the pix_w of v3d_recon_mesh_pixel_weights of the same view.
 * beta_k = w_k / (w_0 + w_1 + w_2) (perspective-correct, sums to 1 by construction, free of the clamped depth);  (u, v) = sum beta_k corner_k,
 * evaluated as corner_0 + beta_1 (corner_1 - corner_0) + beta_2 (corner_2 - corner_0) relative to the cell's origin (du = beta_1 L clamped
 * to 0 .. L and dv = beta_2 L clamped to 0 .. L - du, counted from the right-angle corner: fp32 steps of a coordinate below S, not below R,
 * and a sum that rounding cannot carry past the hypotenuse), which keeps it inside the chart's bounding box [lo, hi];  i0 = min(floor(u), hi_x - 1), j0 likewise, fu = u - i0, fv = v - j0.  pix_tex [H][W][4]: the indices of texels
 * (i0, j0), (i0+1, j0), (i0, j0+1), (i0+1, j0+1);  pix_tw [H][W][4]: (1-fu)(1-fv), fu (1-fv), (1-fu) fv, fu fv.  -1 and 0 where face_id < 0
 * (or is not below F, or the weights do not have a positive sum).  Every index written is inside 0 .. R R - 1 or is -1. */
int v3d_recon_tex_pixel_texels(const int32_t* face_id, const float* pix_w, int32_t num_faces, int32_t tex_size, int32_t width, int32_t height,
                               int32_t* pix_tex, float* pix_tw, v3d_stream_t stream);

/* One thread per pixel: image [3][H][W], image[ch][p] = tw_0 T[t_0][ch] + tw_1 T[t_1][ch] + tw_2 T[t_2][ch] + tw_3 T[t_3][ch] from texture
 * [R R][3];  bg0 bg1 bg2 where pix_tex[p][0] < 0 (or an index is outside the texture: nothing is read through it). */
int v3d_recon_tex_shade(const int32_t* pix_tex, const float* pix_tw, const float* texture, int32_t tex_size, int32_t width, int32_t height, float bg0,
                        float bg1, float bg2, float* image, v3d_stream_t stream);

/* One thread per pixel: four records per covered pixel at rows 4 offsets[pixel] .. + 3 (offsets: exclusive scan of pix_tex[pixel][0] >= 0,
 * num_records = 4 x its total, positive), keys = texel index, vals = 4 pixel + j: in pixel order. */
int v3d_recon_tex_texel_records(const int32_t* pix_tex, const int32_t* offsets, int32_t width, int32_t height, int32_t num_records, uint64_t* keys,
                                uint32_t* vals, v3d_stream_t stream);

/* The transpose of the shade: dL_dtex [num_texels][3] from dL_dimage [3][H][W], dL_dtex[t][ch] = sum over the entries e of texel t of
 * ent_w[e] dL_dimage[ch][ent_pix[e]].  One thread per texel adds its list front to back in fp32.  Every row is written, 0 0 0 for an empty
 * list.  The arguments of v3d_recon_mesh_shade_bwd, which gives the same sums in another order with a 64-lane wave per row: on the
 * documented path most lists are empty and the rest a few entries long.  num_entries may be 0 (ent_pix, ent_w NULL). */
int v3d_recon_tex_shade_bwd(const int32_t* ranges, const int32_t* ent_pix, const float* ent_w, int32_t num_entries, const float* dL_dimage,
                            int32_t width, int32_t height, int32_t num_texels, float* dL_dtex, v3d_stream_t stream);

/* ---- Mesh vertex fit (v3d_amd/csrc_recon/meshdeform.hip; host side: v3d_amd/recon/mesh_deform.py) -----------------------------------------
 * Moves the mesh's vertices so that its silhouette matches alpha maps of known cameras.  Visibility changes with every step, so nothing is
 * frozen: every iteration runs the forward of "Mesh rasterizer" and then
 *   v3d_recon_mesh_aa_alpha -> (loss on the host side) -> v3d_recon_mesh_aa_count -> scan of the counts -> v3d_recon_mesh_aa_emit -> sort of
 *   the records on max(1, bits(V - 1)) key bits -> v3d_recon_mesh_vertex_ranges -> v3d_recon_mesh_aa_reduce -> v3d_recon_mesh_project_bwd
 * (the scan and the sort are v3d_gs_scan and v3d_gs_radix_sort_pairs of libv3d_hip.so, called by the host).  No atomics: the sort is stable,
 * so a vertex's records stay in pixel-then-neighbour-then-corner order, and one wave sums them in an order that the list alone decides.
 *
 * THE PAIR RULE.  A pair is a covered pixel p (face_id >= 0, face f) and one of its four neighbours q (right, left, down, up, in that
 * order) that lies inside the image and has face_id < 0.  With the corners of f in pix_f (float32, unsnapped) and the edge k running from
 * corner k to corner k + 1,  E_k(x) = s cross(v - u, x - u),  s = -1 where the doubled area of the SNAPPED corners (pix_q, int64) is negative
 * and +1 otherwise: the rasterizer's own integer decision.  Every product and every difference of E_k is rounded to float32 on its own.
 * The candidates are the edges with E_k(q) < 0;  for a candidate Ep = max(E_k(p), 0) and t_k = Ep / (Ep - E_k(q));  the pair's t is the
 * smallest t_k, the lower k on equal t_k;  a pair without a candidate contributes nothing.  The pair adds t - 0.5 to its receiver: p when
 * t < 0.5, else q.  A pixel's antialiased alpha is its coverage (1 or 0) plus what it receives, added in float32 in the order of the
 * pixel's own neighbours, clamped to 0 .. 1.  Pairs between two covered pixels are not touched.  A face with an index outside 0 .. V-1 or
 * a marked corner forms no pair. */

/* One thread per pixel, a gather over its four neighbours.  face_id [H][W], faces [F][3], pix_f [V][2], pix_q [V][2]: the forward of the same
 * view (cull = 1).  alpha_aa [H][W]: the clamped sum;  alpha_raw [H][W]: the sum before the clamp (the backward's clamp test). */
int v3d_recon_mesh_aa_alpha(const int32_t* face_id, const int32_t* faces, int32_t num_faces, const float* pix_f, const int32_t* pix_q,
                            int32_t num_verts, int32_t width, int32_t height, float* alpha_aa, float* alpha_raw, v3d_stream_t stream);

/* One thread per pixel.  counts [H][W]: 2 x the number of the pixel's pairs that have a candidate (0 on a background pixel): the records it
 * will emit.  pair_info [H][W][4] or NULL, for inspection: per neighbour -1 where there is no pair, -2 for a pair without a candidate, else
 * the chosen edge k, + 4 when the receiver is the neighbour. */
int v3d_recon_mesh_aa_count(const int32_t* face_id, const int32_t* faces, int32_t num_faces, const float* pix_f, const int32_t* pix_q,
                            int32_t num_verts, int32_t width, int32_t height, int32_t* counts, int32_t* pair_info, v3d_stream_t stream);

/* One thread per pixel: the records of pixel p at rows offsets[p] .. (offsets: exclusive scan of counts, num_records its total, positive), in
 * neighbour order, the chosen edge's corner k before corner k + 1:  keys = vertex, vals = the record's own row, payload [n][2] = the record's
 * dL/dpix_f.  dL/dt is dL_dalpha at the receiver, 0 where alpha_raw there lies outside the open interval (0, 1) or E_k(p) < 0 was clamped;
 * dt/dEp = -Eq / (Ep - Eq)^2, dt/dEq = Ep / (Ep - Eq)^2, dE(x)/du = s (v_y - x_y, x_x - v_x), dE(x)/dv = s (x_y - u_y, u_x - x_x).  Records
 * of value 0 are written too.  alpha_raw: that of v3d_recon_mesh_aa_alpha on the same arguments. */
int v3d_recon_mesh_aa_emit(const int32_t* face_id, const int32_t* faces, int32_t num_faces, const float* pix_f, const int32_t* pix_q, int32_t num_verts,
                           int32_t width, int32_t height, const float* alpha_raw, const float* dL_dalpha, const int32_t* offsets, int32_t num_records,
                           uint64_t* keys, uint32_t* vals, float* payload, v3d_stream_t stream);

/* dL_dpix [V][2] = the sum over the records of every vertex (ranges [V][2] of v3d_recon_mesh_vertex_ranges on the sorted keys, vals_sorted
 * the sorted values) of payload[vals_sorted[e]].  One 64-lane wave per vertex: lane l adds entries start + l, start + l + 64, .. in list
 * order, the lanes then meet in the xor butterfly of v3d_recon_mesh_shade_bwd.  Every row is written, 0 0 for an empty list.  num_records may
 * be 0 (vals_sorted, payload NULL). */
int v3d_recon_mesh_aa_reduce(const int32_t* ranges, const uint32_t* vals_sorted, const float* payload, int32_t num_records, int32_t num_verts,
                             float* dL_dpix, v3d_stream_t stream);

/* One thread per vertex: dL_dverts [V][3] from dL_dpix [V][2] through the statements of v3d_recon_mesh_project, the 1 / (hw + 1e-7) included.
 * A marked vertex (pix_q INT32_MIN) gets 0 0 0. */
int v3d_recon_mesh_project_bwd(const float* verts, int32_t num_verts, const v3d_gs_camera* cam, const int32_t* pix_q, const float* dL_dpix,
                               float* dL_dverts, v3d_stream_t stream);

/* One thread per vertex over the corner lists of "Mesh topology": grad [V][3] = scale x the sum over the vertex's list, in list order, of
 * 2 d_i - d_j - d_k with d_j, d_k the offsets of the face's two other corners: the gradient of sum over faces and their 3 edges of
 * |d_a - d_b|^2 when scale = 2 x the energy's own factor.  offsets [V][3].  0 0 0 for a vertex without faces. */
int v3d_recon_mesh_smooth_grad(const float* offsets, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                               const int32_t* corners, float scale, float* grad, v3d_stream_t stream);

/* ---- Mesh BVH and normal bake (v3d_amd/csrc_recon/meshbvh.hip; host side: v3d_amd/recon/mesh_bake.py) --------------------------------------
 * "What does this ray hit" of one mesh, and with it a normal map of a high-poly mesh baked onto the atlas ("Mesh texture") of a low-poly one.
 *   build:  v3d_recon_bvh_face_keys -> sort of the keys on 30 bits (v3d_gs_radix_sort_pairs, stable: equal codes stay in face order) ->
 *           v3d_recon_bvh_build_nodes -> v3d_recon_bvh_fit_round until a round changes nothing
 *   query:  v3d_recon_bvh_closest_hit;  v3d_recon_tex_bake_normals
 * A linear BVH after Karras 2012.  No atomics.
 *
 * THE NODES.  F faces give 2 F - 1 nodes (2 F - 1 fits int32: F <= 2^30).  Internal nodes are 0 .. F-2, the root is node 0; leaf k (the k-th
 * face in sorted order, face order[k]) is node F - 1 + k; with F = 1 there is no internal node and the lone leaf is the root.
 * left [F-1], right [F-1]: the children of every internal node;  parent [2F-1]: -1 for the root;  lo [2F-1][3], hi [2F-1][3]: the node's
 * axis-aligned box, for a leaf its face's, for an internal node the union of its leaves' (exact: min and max only).  A face with an index
 * outside 0 .. V-1 has the empty box lo = +inf, hi = -inf, which adds nothing to a union, and is never hit.  The tree's height is at most
 * 30 + bits(F - 1): 30 levels of code prefix, then the tie-break below. */
#define V3D_RECON_BVH_STACK 64

/* One thread per face.  face_lo, face_hi [F][3]: the face's box.  keys [F]: the 30-bit Morton code (x in the highest of every three bits) of
 * the box centre 0.5 (lo + hi), every axis quantised to min(floor((c - lo_a) 1024 / (hi_a - lo_a)), 1023), 0 when that is not positive (a NaN
 * centre included) or the mesh has no extent on the axis;  lo_*, hi_*: the bounding box of the mesh's vertices.  vals [F]: the face index. */
int v3d_recon_bvh_face_keys(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, float lo_x, float lo_y, float lo_z,
                            float hi_x, float hi_y, float hi_z, uint64_t* keys, uint32_t* vals, float* face_lo, float* face_hi, v3d_stream_t stream);

/* One thread per sorted position i: it places leaf i (lo, hi of node F - 1 + i from face_lo, face_hi of face order[i]) and, for i < F - 1,
 * builds internal node i: its range of sorted positions by the common-prefix function delta(i, j) = clz(code_i ^ code_j) on the 32-bit words,
 * 32 + clz(i ^ j) where the codes are equal, -1 for j outside 0 .. F-1, and its split;  it writes left[i], right[i] and its children's
 * parent.  parent[0] = -1.  lo, hi of the internal nodes are left for v3d_recon_bvh_fit_round. */
int v3d_recon_bvh_build_nodes(const uint64_t* keys_sorted, const uint32_t* order, const float* face_lo, const float* face_hi, int32_t num_faces,
                              int32_t* left, int32_t* right, int32_t* parent, float* lo, float* hi, v3d_stream_t stream);

/* One thread per internal node (F >= 2), between two buffers done_in, done_out [F-1] (zeros before the first round; a leaf is always done).
 * A node that is done stays done.  A node whose two children are done in done_in writes the union of their boxes, is done in done_out and
 * stores 1 to *changed;  any other node is not done in done_out.  A box written in round r is read from round r + 1 on: no launch reads what
 * it writes.  The host swaps the buffers, runs the rounds in groups with a flag word each, and stops at the first round that stored nothing. */
int v3d_recon_bvh_fit_round(const int32_t* left, const int32_t* right, int32_t num_faces, const int32_t* done_in, int32_t* done_out, float* lo,
                            float* hi, int32_t* changed, v3d_stream_t stream);

/* One thread per ray, 64 to a block, a stack of V3D_RECON_BVH_STACK nodes per ray in LDS.  rays_o, rays_d [N][3]: the direction is used as
 * given, t is in units of it.  Triangle test (Moeller-Trumbore): e1 = v1 - v0, e2 = v2 - v0, p = d x e2, det = e1 . p (0: a miss), s = o - v0,
 * u = (s . p) / det, q = s x e1, v = (d . q) / det, t = (e2 . q) / det;  a hit when u >= 0, v >= 0, u + v <= 1 and tmin <= t <= tmax.  cull,
 * with Ng = e1 x e2: 0 every triangle, 1 only Ng . d < 0, 2 only Ng . d > 0.  The result is the smallest t and, on equal t, the smaller face
 * index;  t [N], face [N], uv [N][2] = (u, v);  a miss gives +inf, -1, 0 0.  The box test is conservative (it never rejects a box the ray
 * enters;  a zero direction component with the origin on a box plane, 0 x inf, puts no constraint on that axis), so only the triangle tests
 * decide the result. */
int v3d_recon_bvh_closest_hit(const float* rays_o, const float* rays_d, float tmin, float tmax, int32_t num_rays, int32_t cull, const int32_t* left,
                              const int32_t* right, const uint32_t* order, const float* lo, const float* hi, const float* verts, int32_t num_verts,
                              const int32_t* faces, int32_t num_faces, float* t, int32_t* face, float* uv, v3d_stream_t stream);

/* One thread per texel of the low mesh's atlas (THE ATLAS above), 64 to a block.  owner [R R] and b0, b1, b2 are those of
 * v3d_recon_tex_bake_vertex_colors.  P = b0 p0 + b1 p1 + b2 p2 from low_verts, n = b0 n0 + b1 n1 + b2 n2 from low_normals, divided by its
 * length ((0, 0, 1) when the squared length is not above 1e-20).  Two casts against the high mesh (the tree, verts, faces above) by the
 * rules of v3d_recon_bvh_closest_hit: from P along +n with cull = 2 and 0 <= t <= max_dist, from P along -n with cull = 1 and
 * 0 < t <= max_dist;  the smaller t wins, +n on equal t.  normal_map [R R][3]: the high mesh's `normals` [V][3] at the hit,
 * (1 - u - v) m0 + u m1 + v m2, divided by its length (the same rule);  n itself where neither cast hits;  (0, 0, 1) on unowned texels and
 * on faces with an index outside the low vertices.  dist [R R]: +t or -t of the chosen hit, NaN without one.  hit_face [R R]: its face, or -1. */
int v3d_recon_tex_bake_normals(const float* low_verts, int32_t low_num_verts, const int32_t* low_faces, int32_t low_num_faces, const float* low_normals,
                               int32_t tex_size, float max_dist, const int32_t* left, const int32_t* right, const uint32_t* order, const float* lo,
                               const float* hi, const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const float* normals,
                               int32_t* owner, float* normal_map, float* dist, int32_t* hit_face, v3d_stream_t stream);

/* ---- Mesh queries (v3d_amd/csrc_recon/meshquery.hip; host side: v3d_amd/recon/mesh_query.py) ------------------------------------------------
 * Three more questions to the tree of "Mesh BVH and normal bake" (THE NODES; the tree arguments come in the order of
 * v3d_recon_bvh_closest_hit): the closest point of the mesh to a point, and with the midpoint samples of a mesh the distance between two
 * meshes;  whether anything lies along a ray, and with a hemisphere of rays per texel an ambient-occlusion map on the atlas of "Mesh texture".
 * No atomics.  Every walk keeps its stack of V3D_RECON_BVH_STACK nodes in LDS, is bounded by the node count and drops a push past the stack.
 *
 * THE CLOSEST POINT OF A TRIANGLE a, b, c to p (the region method; e1 = b - a, e2 = c - a, all in float):
 *   d1 = e1 . (p - a), d2 = e2 . (p - a);            d1 <= 0 and d2 <= 0:              u, v = 0, 0                     (vertex a)
 *   d3 = e1 . (p - b), d4 = e2 . (p - b);            else d3 >= 0 and d4 <= d3:        u, v = 1, 0                     (vertex b)
 *   vc = d1 d4 - d3 d2;                              else vc <= 0, d1 >= 0, d3 <= 0:   u, v = d1 / (d1 - d3), 0        (edge a b)
 *   d5 = e1 . (p - c), d6 = e2 . (p - c);            else d6 >= 0 and d5 <= d6:        u, v = 0, 1                     (vertex c)
 *   vb = d5 d2 - d1 d6;                              else vb <= 0, d2 >= 0, d6 <= 0:   u, v = 0, d2 / (d2 - d6)        (edge a c)
 *   va = d3 d6 - d5 d4, m = d4 - d3, n = d5 - d6;    else va <= 0, m >= 0, n >= 0:     w = m / (m + n); u, v = 1 - w, w  (edge b c)
 *   else, with s = va + vb + vc:                                                       u, v = vb / s, vc / s           (inside)
 * u and v weigh b and c as in the ray query.  The closest point is q = a + u e1 + v e2, but b itself where u == 1 and c itself where v == 1
 * (a + (b - a) is rounded twice: a query at a vertex must be 0 away), and the squared distance is |p - q|^2 computed from q.  A dot product
 * is (x x' + y y') + z z'. */

/* One thread per point, 64 to a block.  points [N][3].  Every triangle tested gives (d2, u, v) by THE CLOSEST POINT OF A TRIANGLE.  Skipped:
 * a face with an index outside 0 .. V-1;  a face with |e1 x e2|^2 == 0, taken as: in every component of e1 x e2 the two products, each
 * rounded on its own, are equal;  a triangle whose d2 is not finite (a sliver whose sums underflow to 0 / 0, or an overflow).  The result is
 * the smallest d2 and, on equal d2, the smaller face index, among the triangles with d2 <= max_dist^2 (closed;  max_dist may be +inf, NaN
 * or a negative value is refused):  dist [N] = sqrtf(d2), face [N], uv [N][2] = (u, v).  A miss, also for a point with a coordinate that
 * is not finite: +inf, -1, 0 0.  A node's bound is the squared distance from p to its box (c = min(max(p, lo), hi) per axis, |p - c|^2);
 * of two children the one with the smaller bound is descended and the other pushed;  a node is skipped only when
 * bound (1 - 2^-18) > best d2, strictly, so a box at exactly the best distance is still visited.  In exact arithmetic only the triangle
 * tests decide the result.  In float they do up to the rounding of d2: q carries an error of a few ulps of the COORDINATES, so for a query
 * much nearer to the surface than the coordinates are large the relative error of d2 can exceed the slack, and a leaf whose computed d2
 * would have tied or won by less than that error can be skipped.  The answer is still a function of the arguments alone (two runs are
 * bit-equal) and within that rounding of the smallest distance;  the smaller-face rule is exact among the triangles tested. */
int v3d_recon_bvh_closest_point(const float* points, int32_t num_points, float max_dist, const int32_t* left, const int32_t* right,
                                const uint32_t* order, const float* lo, const float* hi, const float* verts, int32_t num_verts,
                                const int32_t* faces, int32_t num_faces, float* dist, int32_t* face, float* uv, v3d_stream_t stream);

#define V3D_RECON_SAMPLES_MAX_SUBDIVIDE 16
/* One thread per sample: the midpoint rule over n^2 congruent sub-triangles of every face, n = subdivide in 1 .. 16 (F n^2 must fit int32).
 * Sample f n^2 + k:  for k < n (n + 1) / 2 an upright sub-triangle, k counting rows j = 0 .. n-1 of i = 0 .. n-1-j (i fastest), at
 * b1, b2 = (i + t) / n, (j + t) / n with t = 1/3 rounded to float;  for the other k, k - n (n + 1) / 2 counts rows j = 0 .. n-2 of
 * i = 0 .. n-2-j of inverted sub-triangles, the same with t = 2/3 rounded to float.  points [F n^2][3] = a + b1 e1 + b2 e2;
 * weights [F n^2] = 0.5 sqrtf(|e1 x e2|^2) / n^2: the sub-triangle's area.  A face with an index outside 0 .. V-1: 0 0 0 and weight 0. */
int v3d_recon_mesh_face_samples(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, int32_t subdivide, float* points,
                                float* weights, v3d_stream_t stream);

#define V3D_RECON_OCCLUSION_MAX_SAMPLES 1024
/* One wave (a block of 64 threads) per point;  lane l casts samples k = l, l + 64, ... < K, K = num_samples in 1 .. 1024;  the hits of every
 * round of 64 are counted with a ballot and lane 0 writes hits [N].  points, normals [N][3].  A point with a coordinate that is not finite,
 * or a normal whose squared length is not finite or not above 1e-20: hits = -1, nothing is cast.  n = normal / its length.
 * DIRECTION k OF POINT i, in 32-bit unsigned arithmetic up to the conversion:  h = ((i + 1) 0x9E3779B9) ^ seed, then h ^= h >> 16,
 * h *= 0x85EBCA6B, h ^= h >> 13, h *= 0xC2B2AE35, h ^= h >> 16;  frac = (float)(k 2654435769 + h) / 2^32;  u = (k + 0.5) / K,
 * r = sqrtf(u), z = sqrtf(1 - u);  (sin, cos) of 2 pi frac by sincospif(2 frac);  s = copysignf(1, n.z), a = -1 / (s + n.z), b = n.x n.y a,
 * t1 = (1 + s n.x^2 a, s b, -s n.x), t2 = (b, s + n.y^2 a, -n.y);  d = r cos t1 + r sin t2 + z n: cosine-weighted over the hemisphere of n,
 * so the occlusion is hits / K.  The ray: origin p + bias n, 0 <= t <= radius (finite, > 0;  bias finite, >= 0), cull = 0, the triangle and
 * box tests of v3d_recon_bvh_closest_hit with best = tmax;  the walk returns at the first triangle that is hit: a boolean of the set of
 * triangles, which no order of the walk changes. */
int v3d_recon_bvh_occlusion(const float* points, const float* normals, int32_t num_points, int32_t num_samples, float radius, float bias, uint32_t seed,
                            const int32_t* left, const int32_t* right, const uint32_t* order, const float* lo, const float* hi, const float* verts,
                            int32_t num_verts, const int32_t* faces, int32_t num_faces, int32_t* hits, v3d_stream_t stream);

/* One thread per texel of the atlas (THE ATLAS above): owner [R R], P [R R][3] and n [R R][3] exactly as v3d_recon_tex_bake_normals forms
 * them before it casts (b0, b1, b2 constant across the gutter;  n divided by its length, (0, 0, 1) when the squared length is not above
 * 1e-20).  An unowned texel, and one whose face has an index outside the vertices: P = NaN NaN NaN, n = 0 0 1. */
int v3d_recon_tex_texel_frames(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const float* normals, int32_t tex_size,
                               int32_t* owner, float* positions, float* frame_normals, v3d_stream_t stream);

/* ---- Mesh solid (v3d_amd/csrc_recon/meshsolid.hip; host side: v3d_amd/recon/mesh_solid.py) --------------------------------------------------
 * "Am I inside" of the tree of "Mesh BVH and normal bake" (THE NODES; the tree arguments come in the order of v3d_recon_bvh_closest_hit):
 * the generalized winding number (Jacobson et al. 2013), summed hierarchically with one dipole per node (the first order of Barill et al.
 * 2018), and with the closest point of "Mesh queries" a signed distance and a volume of v3d_recon_tsdf_integrate filled from a mesh, open or closed.
 *   moments:  v3d_recon_bvh_moment_round until a round changes nothing, after the fit's boxes are final
 *   query:    v3d_recon_bvh_winding;  v3d_recon_sdf_grid
 * No atomics.  Every kernel is launched in blocks of one wave;  every walk keeps its stack of V3D_RECON_BVH_STACK nodes in LDS
 * (stack[entry * 64 + lane]), is bounded by the node count and drops a push past the stack.
 *
 * THE WINDING NUMBER.  For a query q and a triangle v0 v1 v2, with a = v0 - q, b = v1 - q, c = v2 - q, all in float:
 *   num = a . (b x c),   den = |a| |b| |c| + (a . b) |c| + (b . c) |a| + (c . a) |b|,   Omega = 2 atan2f(num, den),
 *   Omega = 0 where num == 0 (a query in the triangle's plane: on the triangle, where the angle has no value, and beside it, where it is 0),
 *   Omega = 0 for a face with an index outside 0 .. V-1.   w(q) = sum of Omega over the faces / (4 pi).
 * A triangle wound so that e1 x e2 points outward gives +1 inside a closed mesh, 0 outside;  the same mesh wound inward gives -1 inside.
 * A dot product is (x x' + y y') + z z';  |x| = sqrtf(x . x).
 *
 * THE MOMENTS.  mom [2F-1][8] float, a row per node of THE NODES: (nx, ny, nz, r2, cx, cy, cz, area).
 *   Leaf of a face whose indices are vertices:  n = 0.5 e1 x e2 (e1 = v1 - v0, e2 = v2 - v0);  area = |n|;  c = ((v0 + v1) + v2) / 3.
 *     A face without area as v3d_recon_bvh_closest_point takes it (in every component of e1 x e2 the two products are equal) has n = 0 and
 *     area = 0 exactly, and keeps its c.
 *   Leaf of a face with an index outside 0 .. V-1:  all zeros.
 *   Internal node, from its children l, r:  n = n_l + n_r;  area = a_l + a_r;  c = (a_l c_l + a_r c_r) / area where area > 0, otherwise
 *     the centre 0.5 (lo + hi) of the node's box, or 0 0 0 for the empty box.
 *   Every node:  r2 = (mx + my) + mz with m_k = max((c_k - lo_k)^2, (hi_k - c_k)^2) on the node's own box: the squared distance from c to
 *     the box's farthest corner, a bound on everything below the node;  r2 = 0 for the empty box (lo > hi on an axis).
 *
 * THE SUM.  The walk starts at the root, descends the left child and pushes the right (depth <= height <= V3D_RECON_BVH_STACK), so the
 * order of the sum is a function of the tree alone.  With d = c - q and d2 = d . d:
 *   a node with area == 0 adds nothing and is not descended;
 *   a node, leaf or internal, is FAR when beta^2 > 0 and d2 > beta^2 r2 (beta^2 and the product in float);  it adds (n . d) / (d2 sqrtf(d2));
 *   a leaf that is not far adds its Omega;   an internal node that is not far is opened.
 * beta == 0 never approximates: the sum is THE WINDING NUMBER's own.  Every term is computed in float;  the running sum is a double,
 * divided by 4 pi in double and rounded to float once.  A query with a coordinate that is not finite answers NaN without a walk. */

/* One thread per node, 64 to a block, between two buffers done_in, done_out [2F-1] (zeros before the first round;  unlike the fit's they
 * hold the leaves too).  A node that is done stays done.  A leaf that is not done writes its row of THE MOMENTS (so the first round writes
 * the leaves), an internal node whose two children are done in done_in writes its row from theirs;  both are done in done_out and store 1
 * to *changed;  any other node is not done in done_out.  A row written in round r is read from round r + 1 on: no launch reads a row it
 * writes.  The host runs the rounds as it runs v3d_recon_bvh_fit_round, AFTER the boxes are final (lo, hi are read, never written).  F = 1:
 * one round writes the lone leaf. */
int v3d_recon_bvh_moment_round(const int32_t* left, const int32_t* right, const uint32_t* order, const float* lo, const float* hi, const float* verts,
                               int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* done_in, int32_t* done_out, float* mom,
                               int32_t* changed, v3d_stream_t stream);

/* One thread per query, 64 to a block.  points [N][3];  w [N] by THE SUM with `beta` (finite, >= 0;  0: the exact sum) on mom [2F-1][8]. */
int v3d_recon_bvh_winding(const float* points, int32_t num_points, float beta, const int32_t* left, const int32_t* right, const uint32_t* order,
                          const float* lo, const float* hi, const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces,
                          const float* mom, float* w, v3d_stream_t stream);

/* One thread per voxel of a volume of v3d_recon_tsdf_integrate (voxel (ix, iy, iz) at [iz][iy][ix], N in 2 .. V3D_RECON_MAX_N).  A block of 64 threads is a
 * 4 x 4 x 4 brick: lane l is voxel (4 bx + (l & 3), 4 by + ((l >> 2) & 3), 4 bz + (l >> 4)) of block (bx, by, bz) in a grid of
 * ceil(N / 4)^3;  lanes outside the volume idle.  The result does not depend on this mapping.  The voxel's centre on every axis is
 * fmaf(i + 0.5, voxel, -bound) with voxel = 2 bound / N in float: the exact (i + 0.5) voxel - bound rounded to float once.  Per voxel:
 * the closest point by v3d_recon_bvh_closest_point's rules with max_dist = trunc (closed), then w by THE SUM;  s = -1 where w >= 0.5, else
 * +1 (a NaN w gives +1).  tsdf_sum = s min(dist / trunc, 1), or s on a miss;  weight = 1 always;  on a hit and with colors [V][3] given,
 * rgb_sum [3][N][N][N] = (1 - u - v) c0 + u c1 + v c2 of the closest face's vertex colours and rgb_weight = 1;  on a miss, or with colors
 * NULL (no colour is read), both are 0.  Negative is inside, as v3d_recon_cells_flag takes it.  bound and trunc finite and positive. */
int v3d_recon_sdf_grid(const int32_t* left, const int32_t* right, const uint32_t* order, const float* lo, const float* hi, const float* verts,
                       int32_t num_verts, const int32_t* faces, int32_t num_faces, const float* mom, const float* colors, int32_t resolution, float bound,
                       float trunc, float beta, float* tsdf_sum, float* weight, float* rgb_sum, float* rgb_weight, v3d_stream_t stream);

/* ---- Tangent space and GLB (v3d_amd/csrc_recon/meshtangent.hip; host side: v3d_amd/recon/mesh_gltf.py) ---------------------------------------
 * What a glTF 2.0 file needs beside the atlas of "Mesh texture": per-corner NORMAL and TANGENT frames, the object-space normal map of "Mesh
 * BVH and normal bake" re-expressed in those frames (glTF's normalTexture is in tangent space) and back, and a lit shade of one view from
 * exactly that data.  No atomics, no LDS: a face, a texel and a pixel each belong to one thread.
 *
 * THE TANGENT FRAME.  Atlas texel row y is row y from the top of the written image, so the glTF TEXCOORD_0 of the atlas coordinate (x, y) is
 * ((x + 0.5) / R, (y + 0.5) / R): no flip.  glTF's bitangent is w cross(N, T) and points along DECREASING glTF v.  A face's UV map is affine
 * (THE ATLAS): with e1 = p1 - p0, e2 = p2 - p0 and s = +1 in half 0 (f & 1 == 0), -1 in half 1, dP/du = s e1 / L and dP/dv = s e2 / L.  Both
 * halves have the same orientation: cross(dP/du, dP/dv) = e1 x e2 / L^2 whatever s is, so with N on the side of e1 x e2 and T along dP/du,
 * cross(N, T) points along +dP/dv, which is INCREASING v, wherever the face looks in space.  Hence w = -1 on every corner of every face.
 * (For normals on the OTHER side of the winding, N . (e1 x e2) < 0, the definition gives +1.  The project's vertex normals come from the
 * winding;  w stays -1 for any normals given, and a reader that forms w cross(N, T) as glTF says still decodes exactly what was encoded.)
 *   Per corner (f, k):  n = normals[faces[f][k]];  N = n / |n|, (0, 0, 1) where |n|^2 is not above 1e-20.  t' = s e1 - N (N . s e1);
 *     T = t' / |t'|;  where |t'|^2 is not above 1e-20, T is the t1 of DIRECTION k OF POINT i built from N:  q = copysignf(1, N.z),
 *     a = -1 / (q + N.z), b = N.x N.y a, T = (1 + q N.x^2 a, q b, -q N.x).  w = -1.
 *   Per point of a face with barycentrics b:  vN = sum b_k N_k, vT = sum b_k T_k, neither normalised;  vB = w cross(vN, vT).  (What the
 *     consumers of MikkTSpace tangents do per pixel.)
 *   Decode a map value c:  n = c.x vT + c.y vB + c.z vN, divided by its length;  where |n|^2 is not above 1e-20, vN divided by its length;
 *     where |vN|^2 is not above 1e-20 either, (0, 0, 1).
 *   Encode an object-space vector m, the exact inverse:  det = vT . (vB x vN);  c = (m . (vB x vN), m . (vN x vT), m . (vT x vB)) / det,
 *     divided by its length;  (0, 0, 1) where det is not finite, where |det| <= 1e-12, or where |c|^2 is not above 1e-20 (or is not finite).
 * A dot product is (x x' + y y') + z z'. */
#define V3D_RECON_LIT_MAX_LIGHTS 4

/* One thread per face: corner_normals [3F][3] = N and corner_tangents [3F][4] = (T, w) of THE TANGENT FRAME, corner 3 f + k being place k of
 * face f;  verts [V][3], faces [F][3], normals [V][3] (v3d_recon_mesh_vertex_normals, or any others).  A face with an index outside 0 .. V-1
 * writes (0, 0, 1) and (1, 0, 0, -1) three times;  nothing is read through such an index. */
int v3d_recon_tex_corner_frames(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const float* normals,
                                float* corner_normals, float* corner_tangents, v3d_stream_t stream);

/* One thread per texel of the atlas.  owner [R R] and b0, b1, b2 are those of v3d_recon_tex_bake_vertex_colors (constant across the
 * gutter);  vN, vT, vB from the owner's three rows of corner_normals, corner_tangents (w is read from corner 0's tangent).  tangent_map
 * [R R][3] = the encoding of object_map [R R][3] by THE TANGENT FRAME: float unit vectors, not yet 0.5 c + 0.5.  (0, 0, 1) on unowned
 * texels and on the texels of a face with an index outside 0 .. V-1 (faces is read for that test alone). */
int v3d_recon_tex_encode_tangent(const int32_t* faces, int32_t num_faces, int32_t num_verts, const float* corner_normals, const float* corner_tangents,
                                 const float* object_map, int32_t tex_size, int32_t* owner, float* tangent_map, v3d_stream_t stream);

/* The inverse, with the same arguments and the two maps exchanged: object_map [R R][3] = the decoding of tangent_map [R R][3];  (0, 0, 1)
 * on the same texels.  With the frames of a mesh that has moved since the bake and the old tangent map, this is the new object-space map. */
int v3d_recon_tex_decode_tangent(const int32_t* faces, int32_t num_faces, int32_t num_verts, const float* corner_normals, const float* corner_tangents,
                                 const float* tangent_map, int32_t tex_size, int32_t* owner, float* object_map, v3d_stream_t stream);

/* One thread per pixel, on face_id [H][W], pix_w [H][W][3], pix_tex, pix_tw [H][W][4] of one view (v3d_recon_mesh_render,
 * v3d_recon_mesh_pixel_weights, v3d_recon_tex_pixel_texels).  A pixel is covered when 0 <= face_id < F, w_0 + w_1 + w_2 > 0 and its four
 * texel indices lie inside 0 .. R R - 1.  beta_k = w_k / (w_0 + w_1 + w_2);  vN, vT, vB at beta from the face's corner frames;
 * c = sum_j tw_j C[t_j] from tangent_map [R R][3] (float, as v3d_recon_tex_encode_tangent writes it), (0, 0, 1) when tangent_map is NULL;
 * n = the decoding of c;  albedo = sum_j tw_j A[t_j] from albedo [R R][3];  ao = sum_j tw_j O[t_j] from ao_map [R R], 1 when ao_map is
 * NULL.  image [3][H][W]:  image[ch] = albedo[ch] (ambient ao + sum_k I_k max(0, n . d_k)) over K = num_lights in 0 .. 4 directional lights,
 * d_k = light_dirs[k] (world space, pointing TOWARDS the light, unit: the caller normalises), I_k = light_intensity[k];  not clamped;
 * bg0 bg1 bg2 where the pixel is not covered.  normals [3][H][W]: n, 0 0 0 where the pixel is not covered.  light_dirs [K][3] and
 * light_intensity [K] are HOST arrays, read before the call returns (NULL when K = 0). */
int v3d_recon_tex_shade_lit(const int32_t* face_id, const float* pix_w, const int32_t* pix_tex, const float* pix_tw, int32_t num_faces,
                            const float* corner_normals, const float* corner_tangents, const float* tangent_map, const float* albedo,
                            const float* ao_map, int32_t tex_size, int32_t width, int32_t height, int32_t num_lights, const float* light_dirs,
                            const float* light_intensity, float ambient, float bg0, float bg1, float bg2, float* image, float* normals,
                            v3d_stream_t stream);

/* ---- Mesh remeshing (v3d_amd/csrc_recon/meshremesh.hip; host side: v3d_amd/recon/mesh_remesh.py) -------------------------------------------
 * Isotropic remeshing towards a target edge length L (Botsch & Kobbelt 2004): split the edges longer than hi = 4/3 L, collapse those shorter
 * than lo = 4/5 L, flip edges towards valence 6 (4 on an open edge), relax the vertices in their tangent planes, put them back on the input.
 * THE STATE: verts [Vcap][3], colors [Vcap][3], faces [Fcap][3] and counts [2] = (V_live, F_live) on the device: rows 0 .. V_live-1 and
 * 0 .. F_live-1 have been born.  Every entry is called with num_verts = Vcap and num_faces = Fcap.  A dead or unborn face holds Vcap in all
 * three places (the rule of "Mesh decimation": absent for every entry); an unborn vertex has no face.  Only a split moves the counts.
 *   per round:  the corner lists of "Mesh decimation" (with Vcap + 1 vertices) -> one of the three propose entries -> keys [V], targets [V] ->
 *               v3d_recon_mesh_decim_min_round twice -> v3d_recon_mesh_decim_accept with max_error = +inf -> (split only: v3d_gs_scan of accept,
 *               rank [V + 1]) -> the matching apply entry, which edits the faces IN PLACE
 *   once per iteration:  v3d_recon_remesh_relax between two buffers;  v3d_recon_bvh_closest_point against the tree of the INPUT mesh, then
 *               v3d_recon_remesh_project
 *   at the end: v3d_recon_mesh_compact_faces
 * THE KEY of a proposal by vertex v: fp32 bits of a finite priority >= 0 (smaller is sooner) << 32 | (v * 0x9E3779B1 mod 2^32); all ones for no
 * proposal (targets[v] = -1).  The multiplier is odd, so keys stay distinct; the apply entries read accept[v] and never decode a key.
 * Accepted vertices are at least 3 edges apart, so their one-rings share no vertex and no face; every apply thread reads and writes only
 * faces of its own vertex's list and reads all of them before its first store.  One thread per vertex; no atomics; no local arrays;
 * bit-reproducible.  Squared lengths are float, (dx dx + dy dy) + dz dz; hi^2 = (16/9) (L L) and lo^2 = (16/25) (L L) in float; normal tests
 * are fp64; nothing is contracted.  The valence of a vertex is the number of its faces.  A vertex with more than max_valence faces (3 ..
 * V3D_RECON_MESH_MAX_VALENCE) proposes nothing, and no list longer than that is ever walked to its end.
 * THE EDGE (a, b) IS EDITABLE when exactly one entry of a's list has b as its next corner (the face (a, b, c), c its previous corner) and
 * exactly one has b as its previous corner (the face (b, a, d), d its next corner), and a, b, c, d are four different vertices: an open
 * edge, a non-manifold edge and an edge of a folded pair of faces are never edited. */

/* Split.  a proposes, among its editable edges (a, b) with len^2 > hi^2, the longest; the smaller b among equals.  Priority L L / len^2;
 * targets[a] = b. */
int v3d_recon_remesh_split_propose(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                   const int32_t* corners, float target_edge, int32_t max_valence, uint64_t* keys, int32_t* targets,
                                   v3d_stream_t stream);

/* rank [V + 1]: the exclusive scan of accept with its total.  done = min(total, Vcap - V_live, (Fcap - F_live) / 2) from counts_in [2];
 * counts_out [2] = (V_live + done, F_live + 2 done) (two buffers); flag [1], cleared by the caller, = 1 when total > done: the accepted
 * splits of rank >= done are dropped and nothing is written past a buffer.  For accepted a of rank r < done with editable (a, targets[a]):
 * m = V_live + r gets 0.5 (p_a + p_b) and 0.5 (colour_a + colour_b);  (a, b, c) becomes (a, m, c) in place and (m, b, c) is written to face
 * F_live + 2 r;  (b, a, d) becomes (b, m, d) in place and (m, a, d) is written to face F_live + 2 r + 1. */
int v3d_recon_remesh_split_apply(float* verts, float* colors, int32_t num_verts, int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                 const int32_t* corners, const int32_t* accept, const int32_t* targets, const int32_t* rank,
                                 const int32_t* counts_in, int32_t* counts_out, int32_t* flag, v3d_stream_t stream);

/* Collapse v -> u, the half-edge collapse of "Mesh decimation" (u keeps its position and colour) under the rules of
 * v3d_recon_mesh_decim_propose: v's faces are one closed fan of 3 .. max_valence, the link condition, the valence cap on u,
 * n_before . n_after > 0 in fp64, no repeated face.  And: len^2(v, u) < lo^2, and no neighbour w of v other than u has len^2(u, w) > hi^2.
 * Priority len^2: the shortest valid edge, the smaller u among equals; targets[v] = u. */
int v3d_recon_remesh_collapse_propose(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                      const int32_t* corners, float target_edge, int32_t max_valence, uint64_t* keys, int32_t* targets,
                                      v3d_stream_t stream);

/* For every accepted v: every face of v's list that holds targets[v] dies (Vcap Vcap Vcap), every other names targets[v] in v's place, in
 * place; removed[v] = 1 (removed is otherwise left as it is). */
int v3d_recon_remesh_collapse_apply(int32_t* faces, int32_t num_faces, int32_t num_verts, const int32_t* ranges, const int32_t* corners,
                                    const int32_t* accept, const int32_t* targets, int32_t* removed, v3d_stream_t stream);

/* Flip (a, b) -> (c, d).  The target valence t is 6, or 4 where boundary[x] != 0 (v3d_recon_mesh_boundary_flags).  a with 4 .. max_valence
 * faces proposes an editable edge (a, b) when b has 4 .. max_valence faces, c and d have fewer than max_valence, c and d share no face (c's
 * list is walked), gain = sum |val - t| over a, b, c, d now, minus the same with val(a) - 1, val(b) - 1, val(c) + 1, val(d) + 1, is
 * positive, and both new faces (a, d, c) and (d, b, c) have n_new . n_old > 0 in fp64 with both old faces (a, b, c) and (b, a, d),
 * n = (p1 - p0) x (p2 - p0).  The largest gain, the smaller b among equals; priority (float)(8 - gain); targets[a] = b. */
int v3d_recon_remesh_flip_propose(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                  const int32_t* corners, const int32_t* boundary, int32_t max_valence, uint64_t* keys, int32_t* targets,
                                  v3d_stream_t stream);

/* For every accepted a with editable (a, targets[a]): (a, b, c) becomes (a, d, c) and (b, a, d) becomes (d, b, c) (d takes b's place, c
 * takes a's), in place. */
int v3d_recon_remesh_flip_apply(int32_t* faces, int32_t num_faces, int32_t num_verts, const int32_t* ranges, const int32_t* corners,
                                const int32_t* accept, const int32_t* targets, v3d_stream_t stream);

/* verts_out [V][3] (two buffers): out = p + lambda (d - n (n . d)), d = the umbrella mean of v3d_recon_mesh_smooth_pass minus p, n = the sum of
 * v3d_recon_mesh_vertex_normals divided by its length, n . d = (nx dx + ny dy) + nz dz.  The vertex is copied where boundary[v] != 0, where
 * pinned[v] != 0 (pinned [V] or NULL), where it has no face and where the squared length of the normal sum is not above 1e-20.
 * lambda in 0 .. 1. */
int v3d_recon_remesh_relax(const float* verts_in, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                           const int32_t* corners, const int32_t* boundary, const int32_t* pinned, float lambda, float* verts_out,
                           v3d_stream_t stream);

/* hit_face [V], hit_uv [V][2]: what v3d_recon_bvh_closest_point answered for verts against the tree of the input mesh (src_verts, src_colors
 * [Vs][3], src_faces [Fs][3]).  Per coordinate q = a + u (b - a) + v (c - a), but b itself where u == 1 and c itself where v == 1 (THE
 * CLOSEST POINT OF A TRIANGLE), written to verts [V][3] in place; colors [V][3] likewise from the three colours.  A miss (hit_face outside
 * 0 .. Fs-1, an absent face, u or v outside 0 .. 1) keeps the vertex and its colour. */
int v3d_recon_remesh_project(const int32_t* hit_face, const float* hit_uv, const float* src_verts, const float* src_colors, int32_t src_num_verts,
                             const int32_t* src_faces, int32_t src_num_faces, float* verts, float* colors, int32_t num_verts,
                             v3d_stream_t stream);

/* ---- Mesh check (v3d_amd/csrc_recon/meshcheck.hip; host side: v3d_amd/recon/mesh_check.py) --------------------------------------------------
 * "Is this mesh sound": which pairs of faces pass through each other, on the tree of "Mesh BVH and normal bake" (THE NODES; the tree
 * arguments come in the order of v3d_recon_bvh_closest_hit, and there is no query array: the queries are the mesh's own faces), and how many
 * faces meet at every edge and which way they run, on the corner lists of "Mesh topology".
 *   pairs:   v3d_recon_bvh_self_count -> v3d_gs_scan of n_up -> v3d_recon_bvh_self_emit -> sort on f << 32 | g (v3d_gs_radix_sort_pairs)
 *   census:  the corner lists -> v3d_recon_mesh_edge_census;  v3d_recon_mesh_vertex_census
 * No atomics.  All arithmetic is float, and nothing is contracted: every product is rounded on its own.
 *
 * THE PAIR RULE.  Faces f != g are a pair when (a), (b), (c) and (d) hold.  The rule is always evaluated with the face of the lower index as
 * A = (a0, a1, a2) and the other as B = (b0, b1, b2), so (f, g) and (g, f) are one decision.
 *   (a) Both faces are present (every index in 0 .. V-1) and both have area: not |e1 x e2|^2 == 0, taken as in v3d_recon_bvh_closest_point
 *       (in every component of e1 x e2 the two products, each rounded on its own, are equal), e1 = v1 - v0, e2 = v2 - v0.
 *   (b) Their boxes meet.  A face's box is lo = min, hi = max of its three vertices per axis; two boxes meet when lo_A <= hi_B and
 *       lo_B <= hi_A on all three axes (closed, no slack: a crossing point lies in both exact boxes).
 *   (c) s = the number of (i, j) with A's index i equal to B's index j.  s >= 2 (an edge in common, or the same three vertices): never a
 *       pair.  s == 1, the shared vertex at corner ka of A and kb of B: two tests, in this order: A's edge from corner ka + 1 to ka + 2
 *       (mod 3; the edge opposite the shared vertex) against B, then B's edge from kb + 1 to kb + 2 against A.  s == 0: six tests, in this
 *       order: A's edges a0 a1, a1 a2, a2 a0 against B, then B's edges b0 b1, b1 b2, b2 b0 against A.  A pair when any test holds.
 *   (d) THE EDGE (p, q) AGAINST THE TRIANGLE (a, b, c):  e1 = b - a, e2 = c - a, n = e1 x e2 (a component is u_y w_z - u_z w_y, and so on),
 *       dp = n . (p - a), dq = n . (q - a), a dot product being (x x' + y y') + z z'.  The endpoints lie strictly on opposite sides:
 *       (dp > 0 and dq < 0) or (dp < 0 and dq > 0);  else the test fails.  Then d = q - p and
 *       ta = d . ((b - p) x (c - p)),  tb = d . ((c - p) x (a - p)),  tc = d . ((a - p) x (b - p)).
 *       ta + tb + tc = d . n in exact arithmetic, and the crossing point's barycentrics are ta, tb, tc over d . n, which has the sign of -dp:
 *       the test holds when dp > 0 and ta <= 0, tb <= 0, tc <= 0, or dp < 0 and ta >= 0, tb >= 0, tc >= 0.  No quotient is formed.
 * Not decided by this rule: two faces that overlap in one plane (no endpoint is strictly off the plane), and two faces with an edge in common
 * however sharply they are folded onto each other. */

/* One thread per face, 64 to a block, a stack of V3D_RECON_BVH_STACK nodes per face in LDS.  Thread i takes face f = order[i] (the i-th leaf;
 * order must hold every face once, as v3d_recon_bvh_build_nodes leaves it;  a thread whose order[i] lies outside 0 .. F-1 writes nothing).
 * The walk starts at the root, visits every node whose box meets f's box by (b), descends the left child and pushes the right, and at a
 * leaf with face g != f decides THE PAIR RULE;  it is bounded by the node count and drops a push past the stack.
 * n_all [F]: the partners of f of either index order;  n_up [F]: the partners g > f.  A face that fails (a) has 0 and 0. */
int v3d_recon_bvh_self_count(const int32_t* left, const int32_t* right, const uint32_t* order, const float* lo, const float* hi, const float* verts,
                             int32_t num_verts, const int32_t* faces, int32_t num_faces, int32_t* n_all, int32_t* n_up, v3d_stream_t stream);

/* The same walk.  offsets [F + 1]: the exclusive scan of n_up with its total (v3d_gs_scan);  pairs [num_pairs][2], num_pairs >= 1.  The j-th
 * partner g > f that the walk meets is written as pairs[offsets[f] + j] = (f, g) while offsets[f] + j < min(offsets[f + 1], num_pairs):
 * nothing is written past the buffer or into another face's rows, whatever offsets holds.  The rows come grouped by f in ascending f, and
 * within one f in the order of the walk. */
int v3d_recon_bvh_self_emit(const int32_t* left, const int32_t* right, const uint32_t* order, const float* lo, const float* hi, const float* verts,
                            int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* offsets, int32_t num_pairs, int32_t* pairs,
                            v3d_stream_t stream);

/* THE CENSUS.  A face is COUNTED when it is present and its three indices differ.  An entry of v's list (v3d_recon_mesh_corner_records) at
 * place k of a counted face (i0, i1, i2) has the next neighbour i_(k+1) and the previous neighbour i_(k+2) (mod 3): the face runs
 * v -> next and previous -> v.
 * One thread per corner c = 3 f + k, the half-edge i_k -> i_(k+1) of face f.  It walks i_k's list:  same [3F]: the entries of counted faces
 * whose next neighbour is i_(k+1), the corner's own entry included (the faces that run i_k -> i_(k+1));  opposite [3F]: those whose previous
 * neighbour is i_(k+1) (the faces that run i_(k+1) -> i_k).  A corner of a face that is not counted: -1 and -1. */
int v3d_recon_mesh_edge_census(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                               int32_t* same, int32_t* opposite, v3d_stream_t stream);

/* One thread per vertex v.  For every neighbour u of v in a counted entry of v's list, out = the counted entries whose next neighbour is u and
 * in = those whose previous neighbour is u (same and opposite of the half-edge v -> u).  flags [V], the OR over these edges of
 *   1: out + in == 1 (an open edge);   2: out + in >= 3 (a non-manifold edge);
 *   4: (out == 2 and in == 0) or (in == 2 and out == 0) (two faces that run the same way: the winding is inconsistent);
 * and, only where none of these is set and v's list has at least one present face (counted or not),
 *   8: v's star is not one closed fan by the rule of v3d_recon_mesh_decim_propose (two cones that meet at a point; also a face that names
 *      v twice).
 * 0 for a vertex without faces. */
int v3d_recon_mesh_vertex_census(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                                 int32_t* flags, v3d_stream_t stream);

/* ---- Mesh repair (v3d_amd/csrc_recon/meshrepair.hip; host side: v3d_amd/recon/mesh_repair.py) ---------------------------------------------
 * Acts on what "Mesh check" reports and keeps every triangle it has no reason to touch.  Five passes, each an entry or a few, each reading
 * the corner lists of "Mesh topology" and the outputs of THE CENSUS and of the self-pair walk as they are:
 *   weld:    weld_keys -> sort on z (32 bits), then on x << 32 | y (64 bits) -> weld_heads -> v3d_gs_scan -> weld_first -> weld_remap ->
 *            remap_faces
 *   drop:    the corner lists -> drop_flags -> scan of the kept -> v3d_recon_mesh_compact_faces
 *   orient:  the census -> labels = 2 f, then orient_round between two buffers until a round changes nothing -> orient_conflicts ->
 *            orient_apply;  the host sums every closed patch's signed volume in float64 in face order and flips a negative patch whole
 *   cut:     the census and the pairs -> vertex_open -> trouble -> grow (between two buffers, `grow` times) -> compaction of the rest
 *   fill:    the census of what is left -> vertex_open -> 32 x loop_round between two buffers -> sort of the live vertices on their label ->
 *            v3d_recon_mesh_vertex_ranges -> loop_flags -> scans of the new faces and vertices -> fill_emit
 * (every name above with the prefix v3d_recon_repair_).  One thread per vertex, face or loop.  No atomics: every element has one owner, and
 * the two flag words (changed, nonorient) only ever receive a 1.  Integers everywhere but in three places: coordinates are compared by value
 * (weld), the area rule is that of THE PAIR RULE (a), and a loop's centre is a float64 sum rounded once.  Two runs are bit-equal.  A face with
 * an index outside 0 .. V-1 is absent and nothing is read through such an index;  COUNTED is as in THE CENSUS. */

/* WELD.  Two vertices are one when their three float32 coordinates are equal by value (-0.0 equals +0.0;  the host refuses a coordinate
 * that is not finite).  One thread per vertex: keys_z [V] = the bits of z, keys_xy [V] = the bits of x << 32 | the bits of y, a coordinate
 * equal to zero taken as bits 0;  vals [V] = v.  Two stable sorts (z, then x y) leave equal positions next to each other, indices ascending. */
int v3d_recon_repair_weld_keys(const float* verts, int32_t num_verts, uint64_t* keys_z, uint64_t* keys_xy, uint32_t* vals, v3d_stream_t stream);

/* order [V]: the sorted values.  heads [V]: 1 for i == 0 and where the position of order[i] differs by value from that of order[i - 1] (also
 * where either index lies outside 0 .. V-1), else 0. */
int v3d_recon_repair_weld_heads(const float* verts, int32_t num_verts, const int32_t* order, int32_t* heads, v3d_stream_t stream);

/* offsets [V + 1]: the exclusive scan of heads.  first [V]: first[offsets[i]] = order[i] for every head i: the representative of group
 * offsets[i], its smallest index.  Rows past the number of groups are not written. */
int v3d_recon_repair_weld_first(const int32_t* order, const int32_t* heads, const int32_t* offsets, int32_t num_verts, int32_t* first,
                                v3d_stream_t stream);

/* remap [V]: remap[order[i]] = first[offsets[i + 1] - 1], the representative of i's group (the vertex itself where an index is out of range). */
int v3d_recon_repair_weld_remap(const int32_t* order, const int32_t* offsets, const int32_t* first, int32_t num_verts, int32_t* remap,
                                v3d_stream_t stream);

/* faces_out [F][3] (two buffers): every index of a present face replaced by remap of it;  an absent face is copied. */
int v3d_recon_repair_remap_faces(const int32_t* faces, int32_t num_faces, int32_t num_verts, const int32_t* remap, int32_t* faces_out,
                                 v3d_stream_t stream);

/* DROP.  drop [F], one thread per face, the OR of  1: absent (and nothing else);  2: present and not counted (an index twice);  4: present
 * and without area by THE PAIR RULE (a), e1 = v1 - v0, e2 = v2 - v0;  8: counted, and a present face of a lower index holds the same three
 * indices in any order (the thread walks the list of its smallest index).  A face is dropped when its word is not 0. */
int v3d_recon_repair_drop_flags(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                const int32_t* corners, int32_t* drop, v3d_stream_t stream);

/* ORIENT.  same, opposite [3F] of v3d_recon_mesh_edge_census on the same faces.  The counted faces f and g are ADJACENT across half-edge k of
 * f, i_k -> i_(k+1), when same + opposite == 2 there;  rel = 1 when same == 2 (both run the same way) else 0;  g is the other counted entry
 * of i_k's list whose next (rel = 1) or previous (rel = 0) neighbour is i_(k+1).  One round, one thread per face, between two buffers:
 * labels_out[f] = min(labels_in[f], min over adjacent g of (labels_in[g] XOR rel)), from labels = 2 f.  A thread whose label changed stores 1
 * to changed [1], which the caller cleared.  Plain propagation: the fixed point comes within the face graph's diameter + 1 rounds, and F + 8
 * rounds without one mean broken lists.  At the fixed point label >> 1 is the smallest face of the patch and label & 1 says "flip me
 * relative to that face". */
int v3d_recon_repair_orient_round(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                                  const int32_t* same, const int32_t* opposite, const int32_t* labels_in, int32_t* labels_out, int32_t* changed,
                                  v3d_stream_t stream);

/* nonorient [F], cleared by the caller: nonorient[label[f] >> 1] = 1 for every adjacent pair f, g with equal roots and
 * (label[f] XOR label[g]) & 1 != rel.  Such a patch cannot be given one winding. */
int v3d_recon_repair_orient_conflicts(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                                      const int32_t* same, const int32_t* opposite, const int32_t* labels, int32_t* nonorient, v3d_stream_t stream);

/* faces_out [F][3] (two buffers): places 1 and 2 of face f change places when its root r = labels[f] >> 1 has nonorient[r] == 0 and
 * (labels[f] & 1) XOR (patch_flip[r] != 0) is 1;  patch_flip [F] by root, or NULL for none.  Every other face is copied. */
int v3d_recon_repair_orient_apply(const int32_t* faces, int32_t num_faces, const int32_t* labels, const int32_t* nonorient, const int32_t* patch_flip,
                                  int32_t* faces_out, v3d_stream_t stream);

/* CUT.  An OPEN HALF-EDGE is a corner with same == 1 and opposite == 0: u -> w of the one counted face on its edge.  One thread per vertex u
 * over u's list:  next [V] = w when u has exactly one outgoing open half-edge u -> w, else -1;  bad [V] = 1 when flags[u] (of
 * v3d_recon_mesh_vertex_census) has bit 2, 4 or 8, or u has two or more outgoing open half-edges, else 0. */
int v3d_recon_repair_vertex_open(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                                 const int32_t* same, const int32_t* opposite, const int32_t* flags, int32_t* bad, int32_t* next, v3d_stream_t stream);

/* trouble [F] = 1 for a present face with per_face[f] > 0 (n_all of v3d_recon_bvh_self_count) or a bad vertex, else 0. */
int v3d_recon_repair_trouble(const int32_t* faces, int32_t num_faces, int32_t num_verts, const int32_t* per_face, const int32_t* bad, int32_t* trouble,
                             v3d_stream_t stream);

/* trouble_out [F] (two buffers) = trouble_in, and 1 for every present face one of whose three lists holds a present face g with
 * trouble_in[g] != 0. */
int v3d_recon_repair_grow(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                          const int32_t* trouble_in, int32_t* trouble_out, v3d_stream_t stream);

/* FILL.  From labels = v and jump = next, or -1 where bad[v] != 0 (set by the host), 32 rounds between two buffers of:  with j = jump_in[v] in
 * 0 .. V-1, labels_out[v] = min(labels_in[v], labels_in[j]) and jump_out[v] = jump_in[j];  else the label is copied and the jump is -1.
 * After them a vertex is LIVE when its jump is in range (its chain of next never ends and never meets a bad vertex), and a live vertex's
 * label is the smallest vertex its chain visits. */
int v3d_recon_repair_loop_round(int32_t num_verts, const int32_t* labels_in, const int32_t* jump_in, int32_t* labels_out, int32_t* jump_out,
                                v3d_stream_t stream);

/* members [V]: the vertices sorted (stably) on their label, a vertex that is not live on the key V: within one label they ascend, which is
 * the order of label << 32 | vertex.  loop_ranges [V][2]: v3d_recon_mesh_vertex_ranges of the sorted keys.  One thread per vertex x:
 * state [V] = 0 and length [V] = 0 unless x is live and labels[x] == x;  then length = n, the rows of x's range, and state = 1 (FILLABLE) when
 * 3 <= n <= max_hole_edges and stepping u = next[u] from u = next[x] returns to x after exactly n steps through vertices that are in range,
 * not bad and labelled x;  else state = 2 (left: too long, or x's rows hold a chain that runs into the loop and do not close.  Such a chain
 * whose vertices all lie below the loop's smallest is a label of its own, state 2, and the loop itself is then fillable). */
int v3d_recon_repair_loop_flags(int32_t num_verts, const int32_t* next, const int32_t* bad, const int32_t* labels, const int32_t* jump,
                                const int32_t* loop_ranges, const int32_t* members, int32_t max_hole_edges, int32_t* state, int32_t* length,
                                v3d_stream_t stream);

/* One thread per fillable x, serial over its loop.  face_off, vert_off [V + 1]: the exclusive scans of the loop's new faces (1 when n == 3,
 * else n) and new vertices (0 when n == 3, else 1), so loops come in ascending x.  n == 3: the face (n2, n1, x), n1 = next[x], n2 = next[n1].
 * n > 3: the new vertex m = V + vert_off[x] at new_verts[vert_off[x]] = per coordinate the float64 sum over the loop's members in ascending
 * index, divided by (double)n, rounded once to float32;  new_colors likewise from colors (both NULL for none);  the faces (next[u], u, m)
 * for the members u in ascending order.  new_faces [num_new_faces][3], new_verts, new_colors [num_new_verts][3];  a loop whose rows do not
 * fit the buffers writes nothing. */
int v3d_recon_repair_fill_emit(const float* verts, const float* colors, int32_t num_verts, const int32_t* next, const int32_t* loop_ranges,
                               const int32_t* members, const int32_t* state, const int32_t* length, const int32_t* face_off, const int32_t* vert_off,
                               int32_t num_new_faces, int32_t num_new_verts, int32_t* new_faces, float* new_verts, float* new_colors,
                               v3d_stream_t stream);

/* ---- Mesh alignment (v3d_amd/csrc_recon/meshalign.hip; host side: v3d_amd/recon/mesh_align.py) ---------------------------------------------
 * The hot step of an ICP against the tree of "Mesh BVH and normal bake" (THE NODES; the tree arguments come in the order of
 * v3d_recon_bvh_closest_hit): move every sample by a similarity, find its closest point on the tree's mesh, and reduce the weighted
 * moments of the pairs from which the host solves the next similarity (Umeyama).  No atomics: every block writes one row of sums, a second
 * entry adds the rows in a fixed order.  Two calls with the same arguments are bit-equal.
 *
 * THE BUTTERFLY: a value per lane of a wave becomes their sum on every lane by v += (v of lane ^ o) for o = 32, 16, 8, 4, 2, 1.  Both
 * partners of a step add the same two numbers, and an IEEE sum does not depend on the order of its two operands, so every lane holds the
 * same double after every step. */

#define V3D_RECON_ALIGN_COLUMNS 20
/* One thread per sample, 64 to a block (one wave);  the walk's stack lives in LDS as in "Mesh queries".  points [N][3], weights [N].
 * xf [12] is read on the HOST before the call returns: a row-major 3 x 4 float matrix M = [s R | t].
 * Per sample, in float:  p'_r = ((M_r0 x + M_r1 y) + M_r2 z) + M_r3  for the rows r = 0, 1, 2 (whether a product and the sum after it are
 * contracted into one fused operation is the compiler's choice).  The closest point of the tree's mesh to p' is that of
 * v3d_recon_bvh_closest_point with this max_dist (closed;  +inf allowed;  NaN or a negative value is refused), with exactly its rules, ties
 * and misses;  a p' with a coordinate that is not finite is a miss (a sample with a coordinate that is not finite gives such a p').
 * q = a + u e1 + v e2 of the face found, b itself where u == 1 and c itself where v == 1, as THE CLOSEST POINT OF A TRIANGLE forms it.
 * Every sample writes  moved [N][3] = p',  closest [N][3] = q,  dist [N],  face [N],  uv [N][2];  a miss writes q = NaN NaN NaN, +inf, -1
 * and 0 0.  None of these depends on the weight.
 * A sample is VALID when the three coordinates of p' are finite and its weight is finite and >= 0.  It COUNTS when it is valid and not a
 * miss.  Every block writes one row of partials [ceil(N / 64)][20] in double.  Every term is formed in double from the floats above, each
 * operation rounded on its own (no contraction), products from the left:  (w q_i) p'_j,  w ((x x + y y) + z z),  w (dist dist).  A sample
 * that does not count, and a lane past N, adds exact zeros.  The 64 terms of a column are summed by THE BUTTERFLY.
 *   column 0: sum w          1-3: sum w p'         4-6: sum w q          7-15: sum w q_i p'_j at 7 + 3 i + j
 *   16: sum w |p'|^2         17: sum w dist^2      18: the samples that count
 *   19: sum w over all valid samples, counted or not */
int v3d_recon_align_correspond(const float* points, const float* weights, int32_t num_points, const float* xf, float max_dist, const int32_t* left,
                               const int32_t* right, const uint32_t* order, const float* lo, const float* hi, const float* verts, int32_t num_verts,
                               const int32_t* faces, int32_t num_faces, float* moved, float* closest, float* dist, int32_t* face, float* uv,
                               double* partials, v3d_stream_t stream);

/* One block of 64 threads.  partials [num_rows][20], num_rows >= 1.  Lane l adds the rows l, l + 64, ... in increasing order, column by
 * column, from 0.0;  THE BUTTERFLY over the lanes then gives sums [20]. */
int v3d_recon_align_reduce(const double* partials, int32_t num_rows, double* sums, v3d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
