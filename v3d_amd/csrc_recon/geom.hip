// Geometry from the reconstructed splats (include/v3d_recon.h, libv3d_recon.so; host side: v3d_amd/recon/geometry.py): per-pixel expected
// depth and accumulated alpha over the rasterizer's sorted tile lists, TSDF integration of one view, and a table-free surface extraction
// (naive surface nets).  Forward only.  A library of its own: nothing here is linked into libv3d_hip.so, whose v3d_gs_* forward produces the
// inputs of the depth pass and whose v3d_gs_scan the host calls between the extraction passes.
//
// Determinism: no atomics.  A pixel, a voxel, a cell and a grid edge each belong to one thread; compaction goes through exclusive scans.
// Built without -ffast-math (v3d_amd/build.py): the maps are held to an fp64 restatement (tests/recon_geom_ref.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "recon_host.h"
#include "v3d_recon.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------------------
// Depth / alpha.  The alpha evaluation is the colour pass's (gs.hip splat_alpha), statement for statement: the same skip decisions.
__global__ void __launch_bounds__(NT) depth_alpha_kernel(const int32_t* __restrict__ ranges, const uint32_t* __restrict__ gid,
                                                         const float* __restrict__ means2d, const float* __restrict__ conic_op,
                                                         const float* __restrict__ zview, const int32_t* __restrict__ n_contrib, int W, int H,
                                                         int gx, float* __restrict__ out_depth, float* __restrict__ out_alpha) {
    __shared__ float2 s_xy[NT];
    __shared__ float4 s_co[NT];
    __shared__ float s_z[NT];
    const int tile = blockIdx.x, t = threadIdx.x;
    const int px = (tile % gx) * TILE + (t % TILE), py = (tile / gx) * TILE + (t / TILE);
    const bool inside = px < W && py < H;
    const long long pix = (long long)py * W + px;
    const float pxf = (float)px, pyf = (float)py;
    const int start = ranges[2 * tile], end = ranges[2 * tile + 1];
    const int mine = inside ? n_contrib[pix] : 0;      // entries of the tile list this pixel walks: up to its last colour contributor
    int seen = 0;
    float T = 1.f, D = 0.f;
    for (int base = start; base < end; base += NT) {
        if (__syncthreads_count(seen < mine) == 0) break;
        if (base + t < end) {
            const uint32_t g = gid[base + t];
            s_xy[t] = make_float2(means2d[2 * g], means2d[2 * g + 1]);
            s_co[t] = make_float4(conic_op[4 * g], conic_op[4 * g + 1], conic_op[4 * g + 2], conic_op[4 * g + 3]);
            s_z[t] = zview[g];
        }
        __syncthreads();
        const int cnt = min(NT, end - base);
        for (int j = 0; j < cnt && seen < mine; ++j, ++seen) {
            const float2 xy = s_xy[j];
            const float4 co = s_co[j];
            const float dx = xy.x - pxf;
            const float dy = xy.y - pyf;
            const float power = -0.5f * (co.x * dx * dx + co.z * dy * dy) - co.y * dx * dy;
            const float G = expf(power);
            const float alpha = fminf(0.99f, co.w * G);
            if (power > 0.f || alpha < 1.f / 255.f) continue;
            D += s_z[j] * alpha * T;
            T = T * (1.f - alpha);
        }
    }
    if (inside) {
        out_depth[pix] = D;
        out_alpha[pix] = 1.f - T;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// TSDF
__device__ __forceinline__ float voxel_centre(int i, int N, float bound) { return ((float)i + 0.5f) * (2.f * bound / (float)N) - bound; }

__global__ void __launch_bounds__(NT) tsdf_integrate_kernel(const float* __restrict__ depth_map, const float* __restrict__ alpha_map,
                                                            const float* __restrict__ image, v3d_gs_camera cam, int N, float bound, float trunc,
                                                            float alpha_min, float* __restrict__ tsdf_sum, float* __restrict__ weight,
                                                            float* __restrict__ rgb_sum, float* __restrict__ rgb_weight) {
    const int n3 = N * N * N;
    const long long vl = (long long)blockIdx.x * NT + threadIdx.x;
    if (vl >= n3) return;
    const int v = (int)vl;
    const int ix = v % N, iy = (v / N) % N, iz = v / (N * N);
    const float x = voxel_centre(ix, N, bound), y = voxel_centre(iy, N, bound), z = voxel_centre(iz, N, bound);
    const float* V = cam.view;
    const float* P = cam.proj;
    const float zv = x * V[2] + y * V[6] + z * V[10] + V[14];
    if (!(zv > 0.2f)) return;
    const float hx = x * P[0] + y * P[4] + z * P[8] + P[12];
    const float hy = x * P[1] + y * P[5] + z * P[9] + P[13];
    const float hw = x * P[3] + y * P[7] + z * P[11] + P[15];
    const float pw = 1.f / (hw + 0.0000001f);
    const int W = cam.width, H = cam.height;
    const float fx = ((hx * pw + 1.f) * (float)W - 1.f) * 0.5f, fy = ((hy * pw + 1.f) * (float)H - 1.f) * 0.5f;
    const float rx = floorf(fx + 0.5f), ry = floorf(fy + 0.5f);        // nearest pixel
    if (!(rx >= 0.f && rx < (float)W && ry >= 0.f && ry < (float)H)) return;      // (also refuses NaN)
    const long long pix = (long long)(int)ry * W + (int)rx, HW = (long long)H * W;
    const float a = alpha_map[pix];
    if (a < alpha_min || !(a > 0.f)) {        // the view sees through this voxel: empty
        tsdf_sum[v] += 1.f;
        weight[v] += 1.f;
        return;
    }
    const float sdf = depth_map[pix] / a - zv;
    if (sdf < -trunc) return;   // far behind the surface: this view says nothing
    tsdf_sum[v] += fminf(1.f, sdf / trunc);
    weight[v] += 1.f;
    if (fabsf(sdf) <= trunc) {
        for (int ch = 0; ch < 3; ++ch) rgb_sum[(long long)ch * n3 + v] += image[ch * HW + pix];
        rgb_weight[v] += 1.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Surface nets
__device__ __forceinline__ int corner_voxel(int cx, int cy, int cz, int c, int N) {     // corner c: bit 0 = +x, bit 1 = +y, bit 2 = +z
    return ((cz + ((c >> 2) & 1)) * N + cy + ((c >> 1) & 1)) * N + cx + (c & 1);
}

__global__ void __launch_bounds__(NT) cells_flag_kernel(const float* __restrict__ tsdf_sum, const float* __restrict__ weight, int N,
                                                        int32_t* __restrict__ flags) {
    const int M = N - 1, m3 = M * M * M;
    const long long cl = (long long)blockIdx.x * NT + threadIdx.x;
    if (cl >= m3) return;
    const int c = (int)cl;
    const int cx = c % M, cy = (c / M) % M, cz = c / (M * M);
    bool all_seen = true;
    int neg = 0;
    for (int k = 0; k < 8; ++k) {
        const int v = corner_voxel(cx, cy, cz, k, N);
        const float w = weight[v];
        all_seen = all_seen && w > 0.f;
        neg += (w > 0.f && tsdf_sum[v] / w < 0.f) ? 1 : 0;
    }
    flags[c] = (all_seen && neg > 0 && neg < 8) ? 1 : 0;
}

__global__ void __launch_bounds__(NT) cells_vertices_kernel(const float* __restrict__ tsdf_sum, const float* __restrict__ weight,
                                                            const float* __restrict__ rgb_sum, const float* __restrict__ rgb_weight, int N,
                                                            float bound, const int32_t* __restrict__ flags, const int32_t* __restrict__ offsets,
                                                            float* __restrict__ verts, float* __restrict__ colors) {
    const int M = N - 1, m3 = M * M * M, n3 = N * N * N;
    const long long cl = (long long)blockIdx.x * NT + threadIdx.x;
    if (cl >= m3) return;
    const int c = (int)cl;
    if (!flags[c]) return;
    const int cx = c % M, cy = (c / M) % M, cz = c / (M * M);
    float m[8];
    float col[3] = {0.f, 0.f, 0.f};
    int ncol = 0;
    for (int k = 0; k < 8; ++k) {
        const int v = corner_voxel(cx, cy, cz, k, N);
        m[k] = tsdf_sum[v] / weight[v];
        const float cw = rgb_weight[v];
        if (cw > 0.f) {
            for (int ch = 0; ch < 3; ++ch) col[ch] += rgb_sum[(long long)ch * n3 + v] / cw;
            ++ncol;
        }
    }
    // the 12 edges: corner k and corner k | (1 << axis) for every k with that bit clear; positions in cell units (0 .. 1 per axis)
    float p[3] = {0.f, 0.f, 0.f};
    int ncross = 0;
    for (int axis = 0; axis < 3; ++axis)
        for (int k = 0; k < 8; ++k) {
            if (k & (1 << axis)) continue;
            const float m0 = m[k], m1 = m[k | (1 << axis)];
            if ((m0 < 0.f) == (m1 < 0.f)) continue;
            const float s = m0 / (m0 - m1);
            for (int d = 0; d < 3; ++d) p[d] += d == axis ? s : (float)((k >> d) & 1);
            ++ncross;
        }
    const float voxel = 2.f * bound / (float)N;
    const int o = offsets[c];
    const int cc[3] = {cx, cy, cz};
    for (int d = 0; d < 3; ++d) {
        verts[3 * (long long)o + d] = voxel_centre(cc[d], N, bound) + p[d] / (float)ncross * voxel;
        colors[3 * (long long)o + d] = ncol ? col[d] / (float)ncol : 0.5f;
    }
}

// grid edge e = axis * N^3 + v: the 4 cells around it, in counter-clockwise order seen from +axis (u = axis + 1, w = axis + 2, cyclic):
// (u-1, w-1), (u, w-1), (u, w), (u-1, w).  False when the edge is not interior (a cell index would leave 0 .. N-2).
__device__ __forceinline__ bool edge_cells(int e, int N, int& v, int cells[4]) {
    const int n3 = N * N * N, M = N - 1;
    const int axis = e / n3;
    v = e - axis * n3;
    int i[3] = {v % N, (v / N) % N, v / (N * N)};
    const int u = (axis + 1) % 3, w = (axis + 2) % 3;
    if (i[axis] >= M || i[u] < 1 || i[u] >= M || i[w] < 1 || i[w] >= M) return false;
    const int du[4] = {-1, 0, 0, -1}, dw[4] = {-1, -1, 0, 0};
    for (int q = 0; q < 4; ++q) {
        int c[3];
        c[axis] = i[axis];
        c[u] = i[u] + du[q];
        c[w] = i[w] + dw[q];
        cells[q] = (c[2] * M + c[1]) * M + c[0];
    }
    return true;
}

__device__ __forceinline__ int axis_stride(int axis, int N) { return axis == 0 ? 1 : (axis == 1 ? N : N * N); }

__global__ void __launch_bounds__(NT) edges_flag_kernel(const float* __restrict__ tsdf_sum, const float* __restrict__ weight, int N,
                                                        const int32_t* __restrict__ cell_flags, int32_t* __restrict__ flags) {
    const int n3 = N * N * N;
    const long long el = (long long)blockIdx.x * NT + threadIdx.x;
    if (el >= 3LL * n3) return;
    const int e = (int)el;
    int v, cells[4];
    int f = 0;
    if (edge_cells(e, N, v, cells) && cell_flags[cells[0]] && cell_flags[cells[1]] && cell_flags[cells[2]] && cell_flags[cells[3]]) {
        // (flagged cells have weight > 0 on all their corners, the edge's two voxels among them)
        const int v1 = v + axis_stride(e / n3, N);
        f = ((tsdf_sum[v] / weight[v] < 0.f) != (tsdf_sum[v1] / weight[v1] < 0.f)) ? 1 : 0;
    }
    flags[e] = f;
}

__global__ void __launch_bounds__(NT) edges_faces_kernel(const float* __restrict__ tsdf_sum, const float* __restrict__ weight, int N,
                                                         const int32_t* __restrict__ cell_offsets, const int32_t* __restrict__ edge_flags,
                                                         const int32_t* __restrict__ edge_offsets, int32_t* __restrict__ faces) {
    const int n3 = N * N * N;
    const long long el = (long long)blockIdx.x * NT + threadIdx.x;
    if (el >= 3LL * n3) return;
    const int e = (int)el;
    if (!edge_flags[e]) return;
    int v, cells[4];
    if (!edge_cells(e, N, v, cells)) return;
    const int a = cell_offsets[cells[0]], b = cell_offsets[cells[1]], c = cell_offsets[cells[2]], d = cell_offsets[cells[3]];
    const bool up = tsdf_sum[v] / weight[v] < 0.f;     // negative at the lower voxel: the surface faces +axis, counter-clockwise seen from there
    int32_t* f = faces + 6 * (long long)edge_offsets[e];
    f[0] = a; f[1] = up ? b : c; f[2] = up ? c : b;
    f[3] = a; f[4] = up ? c : d; f[5] = up ? d : c;
}

bool volume_ok(int32_t N) { return N >= 2 && N <= V3D_RECON_MAX_N; }

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int v3d_recon_abi_version(void) { return V3D_RECON_ABI_VERSION; }
extern "C" const char* v3d_recon_last_error(void) { return recon_host::g_err; }

extern "C" int v3d_recon_depth_alpha(const int32_t* ranges, const uint32_t* vals_sorted, const float* means2d, const float* conic_opacity,
                                     const float* depth, const int32_t* n_contrib, int32_t width, int32_t height, float* out_depth, float* out_alpha,
                                     v3d_stream_t stream) {
    RECON_REQUIRE(ranges && means2d && conic_opacity && depth && n_contrib && out_depth && out_alpha, "v3d_recon_depth_alpha: null argument");
    RECON_REQUIRE(width > 0 && height > 0, "v3d_recon_depth_alpha: width and height must be positive");
    const int gx = (width + TILE - 1) / TILE, gy = (height + TILE - 1) / TILE;
    RECON_REQUIRE((long long)gx * gy <= 0x7fffffffLL, "v3d_recon_depth_alpha: too many tiles");
    hipLaunchKernelGGL(depth_alpha_kernel, dim3(gx * gy), dim3(NT), 0, ST, ranges, vals_sorted, means2d, conic_opacity, depth, n_contrib, (int)width,
                       (int)height, gx, out_depth, out_alpha);
    return check_launch("v3d_recon_depth_alpha");
}

extern "C" int v3d_recon_tsdf_integrate(const float* depth_map, const float* alpha_map, const float* image, const v3d_gs_camera* cam, int32_t N,
                                        float bound, float trunc, float alpha_min, float* tsdf_sum, float* weight, float* rgb_sum, float* rgb_weight,
                                        v3d_stream_t stream) {
    RECON_REQUIRE(depth_map && alpha_map && image && cam && tsdf_sum && weight && rgb_sum && rgb_weight, "v3d_recon_tsdf_integrate: null argument");
    RECON_REQUIRE(volume_ok(N), "v3d_recon_tsdf_integrate: resolution %d outside 2 .. %d (voxel indices are int32)", (int)N, V3D_RECON_MAX_N);
    RECON_REQUIRE(bound > 0.f && trunc > 0.f, "v3d_recon_tsdf_integrate: bound and trunc must be positive");
    RECON_REQUIRE(cam->width > 0 && cam->height > 0, "v3d_recon_tsdf_integrate: bad camera (positive width and height)");
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(nblk((long long)N * N * N)), dim3(NT), 0, ST, depth_map, alpha_map, image, *cam, (int)N, bound, trunc,
                       alpha_min, tsdf_sum, weight, rgb_sum, rgb_weight);
    return check_launch("v3d_recon_tsdf_integrate");
}

extern "C" int v3d_recon_cells_flag(const float* tsdf_sum, const float* weight, int32_t N, int32_t* flags, v3d_stream_t stream) {
    RECON_REQUIRE(tsdf_sum && weight && flags, "v3d_recon_cells_flag: null argument");
    RECON_REQUIRE(volume_ok(N), "v3d_recon_cells_flag: resolution %d outside 2 .. %d (voxel indices are int32)", (int)N, V3D_RECON_MAX_N);
    const long long M = N - 1;
    hipLaunchKernelGGL(cells_flag_kernel, dim3(nblk(M * M * M)), dim3(NT), 0, ST, tsdf_sum, weight, (int)N, flags);
    return check_launch("v3d_recon_cells_flag");
}

extern "C" int v3d_recon_cells_vertices(const float* tsdf_sum, const float* weight, const float* rgb_sum, const float* rgb_weight, int32_t N,
                                        float bound, const int32_t* flags, const int32_t* offsets, float* verts, float* colors, v3d_stream_t stream) {
    RECON_REQUIRE(tsdf_sum && weight && rgb_sum && rgb_weight && flags && offsets && verts && colors, "v3d_recon_cells_vertices: null argument");
    RECON_REQUIRE(volume_ok(N), "v3d_recon_cells_vertices: resolution %d outside 2 .. %d (voxel indices are int32)", (int)N, V3D_RECON_MAX_N);
    RECON_REQUIRE(bound > 0.f, "v3d_recon_cells_vertices: bound must be positive");
    const long long M = N - 1;
    hipLaunchKernelGGL(cells_vertices_kernel, dim3(nblk(M * M * M)), dim3(NT), 0, ST, tsdf_sum, weight, rgb_sum, rgb_weight, (int)N, bound, flags, offsets,
                       verts, colors);
    return check_launch("v3d_recon_cells_vertices");
}

extern "C" int v3d_recon_edges_flag(const float* tsdf_sum, const float* weight, int32_t N, const int32_t* cell_flags, int32_t* flags,
                                    v3d_stream_t stream) {
    RECON_REQUIRE(tsdf_sum && weight && cell_flags && flags, "v3d_recon_edges_flag: null argument");
    RECON_REQUIRE(volume_ok(N), "v3d_recon_edges_flag: resolution %d outside 2 .. %d (voxel indices are int32)", (int)N, V3D_RECON_MAX_N);
    hipLaunchKernelGGL(edges_flag_kernel, dim3(nblk(3LL * N * N * N)), dim3(NT), 0, ST, tsdf_sum, weight, (int)N, cell_flags, flags);
    return check_launch("v3d_recon_edges_flag");
}

extern "C" int v3d_recon_edges_faces(const float* tsdf_sum, const float* weight, int32_t N, const int32_t* cell_offsets, const int32_t* edge_flags,
                                     const int32_t* edge_offsets, int32_t* faces, v3d_stream_t stream) {
    RECON_REQUIRE(tsdf_sum && weight && cell_offsets && edge_flags && edge_offsets && faces, "v3d_recon_edges_faces: null argument");
    RECON_REQUIRE(volume_ok(N), "v3d_recon_edges_faces: resolution %d outside 2 .. %d (voxel indices are int32)", (int)N, V3D_RECON_MAX_N);
    hipLaunchKernelGGL(edges_faces_kernel, dim3(nblk(3LL * N * N * N)), dim3(NT), 0, ST, tsdf_sum, weight, (int)N, cell_offsets, edge_flags, edge_offsets,
                       faces);
    return check_launch("v3d_recon_edges_faces");
}
