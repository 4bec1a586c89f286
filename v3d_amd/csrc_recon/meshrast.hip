// Triangle rasterizer for the extracted mesh (include/v3d_recon.h "Mesh rasterizer", libv3d_recon.so; host side: v3d_amd/recon/mesh_render.py).
// Forward only.  project (one thread per vertex) -> face_setup (one thread per face) -> v3d_gs_scan -> duplicate_keys -> v3d_gs_radix_sort_pairs
// -> tile_ranges -> render (one 256-thread block per 16 x 16 tile, one pixel per thread, faces staged through LDS in batches of 256): the
// binning of the splat rasterizer (csrc/gs.hip) on triangles.  The scan and the sort are libv3d_hip.so's, called by the host.
//
// Coverage is decided on integers alone: vertices are snapped to a fixed-point grid of 2^subpixel_bits steps per pixel and the three edge
// functions are int64.  Depth and colour are fp32.  No atomics: a vertex, a face, a list entry and a pixel each belong to one thread.
// Built without -ffast-math (v3d_amd/build.py): depth and colour are held to an fp64 restatement (tests/mesh_render_ref.py).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "recon_host.h"
#include "v3d_recon.h"

namespace {

constexpr float Q_LIMIT = 268435456.f;      // 2^28 sub-pixel steps: beyond it a vertex is marked (header: "Mesh rasterizer")
constexpr int MARK = INT32_MIN;

// ---------------------------------------------------------------------------------------------------------------------------------------
// Projection.  View z and the pixel position are tsdf_integrate_kernel's (geom.hip), statement for statement.
__global__ void __launch_bounds__(NT) mesh_project_kernel(const float* __restrict__ verts, int nv, v3d_gs_camera cam, int bits,
                                                          float* __restrict__ out_zv, float* __restrict__ pix_f, int32_t* __restrict__ pix_q) {
    const long long vl = (long long)blockIdx.x * NT + threadIdx.x;
    if (vl >= nv) return;
    const float x = verts[3 * vl], y = verts[3 * vl + 1], z = verts[3 * vl + 2];
    const float* V = cam.view;
    const float* P = cam.proj;
    const float zv = x * V[2] + y * V[6] + z * V[10] + V[14];
    const float hx = x * P[0] + y * P[4] + z * P[8] + P[12];
    const float hy = x * P[1] + y * P[5] + z * P[9] + P[13];
    const float hw = x * P[3] + y * P[7] + z * P[11] + P[15];
    const float pw = 1.f / (hw + 0.0000001f);
    const int W = cam.width, H = cam.height;
    const float fx = ((hx * pw + 1.f) * (float)W - 1.f) * 0.5f, fy = ((hy * pw + 1.f) * (float)H - 1.f) * 0.5f;
    const float S = (float)(1 << bits);
    const float sx = rintf(fx * S), sy = rintf(fy * S);        // (a power of two: the product is exact)
    const bool ok = zv > 0.2f && fabsf(sx) < Q_LIMIT && fabsf(sy) < Q_LIMIT;       // (false on NaN and on infinities)
    out_zv[vl] = zv;
    pix_f[2 * vl] = fx;
    pix_f[2 * vl + 1] = fy;
    pix_q[2 * vl] = ok ? (int)sx : MARK;
    pix_q[2 * vl + 1] = ok ? (int)sy : MARK;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Faces.  A face's snapped corners, its doubled signed area and the pixel centres its bounding box holds.
struct FaceQ {
    int i[3];
    int x[3], y[3];
};

// false when an index lies outside the vertex array or a corner is marked
__device__ __forceinline__ bool face_corners(const int32_t* __restrict__ faces, int f, const int32_t* __restrict__ pix_q, int nv, FaceQ& q) {
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        q.i[k] = faces[3 * (long long)f + k];
        ok = ok && q.i[k] >= 0 && q.i[k] < nv;
    }
    if (!ok) return false;
    for (int k = 0; k < 3; ++k) {
        q.x[k] = pix_q[2 * (long long)q.i[k]];
        q.y[k] = pix_q[2 * (long long)q.i[k] + 1];
        ok = ok && q.x[k] != MARK;
    }
    return ok;
}

__device__ __forceinline__ long long area2(const FaceQ& q) {       // |coordinates| < 2^28: differences < 2^29, products < 2^58
    return (long long)(q.x[1] - q.x[0]) * (q.y[2] - q.y[0]) - (long long)(q.y[1] - q.y[0]) * (q.x[2] - q.x[0]);
}

// pixel (i, j) has its centre at coordinate (i, j), sub-pixel (i << bits, j << bits): the centres inside the bounding box, clamped to the image
__device__ __forceinline__ bool face_rect(const FaceQ& q, int W, int H, int bits, int& x0, int& x1, int& y0, int& y1) {
    const int one = (1 << bits) - 1;
    x0 = max((min(q.x[0], min(q.x[1], q.x[2])) + one) >> bits, 0);         // ceil; >> of a negative int is arithmetic (floor)
    x1 = min(max(q.x[0], max(q.x[1], q.x[2])) >> bits, W - 1);
    y0 = max((min(q.y[0], min(q.y[1], q.y[2])) + one) >> bits, 0);
    y1 = min(max(q.y[0], max(q.y[1], q.y[2])) >> bits, H - 1);
    return x0 <= x1 && y0 <= y1;
}

__global__ void __launch_bounds__(NT) mesh_face_setup_kernel(const int32_t* __restrict__ faces, int nf, const int32_t* __restrict__ pix_q,
                                                             const float* __restrict__ zv, int nv, int W, int H, int bits, int cull,
                                                             int32_t* __restrict__ tiles_touched, float* __restrict__ zmin) {
    const long long fl = (long long)blockIdx.x * NT + threadIdx.x;
    if (fl >= nf) return;
    const int f = (int)fl;
    FaceQ q;
    int tiles = 0;
    float zm = 0.f;
    if (face_corners(faces, f, pix_q, nv, q)) {
        zm = fminf(zv[q.i[0]], fminf(zv[q.i[1]], zv[q.i[2]]));
        const long long a2 = area2(q);
        int x0, x1, y0, y1;
        // front: the outward normal looks at the camera.  View axes are x right, y down, z forward (right-handed), pixels run the same way, so
        // a counter-clockwise face seen from outside has a NEGATIVE doubled area (b - a) x (c - a) in pixel coordinates.
        if (a2 != 0 && !(cull && a2 > 0) && face_rect(q, W, H, bits, x0, x1, y0, y1))
            tiles = (x1 / TILE - x0 / TILE + 1) * (y1 / TILE - y0 / TILE + 1);
    }
    tiles_touched[f] = tiles;
    zmin[f] = zm;
}

__global__ void __launch_bounds__(NT) mesh_duplicate_keys_kernel(const int32_t* __restrict__ faces, int nf, const int32_t* __restrict__ pix_q,
                                                                 int nv, const int32_t* __restrict__ tiles_touched,
                                                                 const int32_t* __restrict__ offsets, const float* __restrict__ zmin, int W, int H,
                                                                 int bits, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
    const long long fl = (long long)blockIdx.x * NT + threadIdx.x;
    if (fl >= nf) return;
    const int f = (int)fl;
    const int n = tiles_touched[f];
    if (n <= 0) return;
    FaceQ q;
    int x0, x1, y0, y1;
    if (!face_corners(faces, f, pix_q, nv, q) || !face_rect(q, W, H, bits, x0, x1, y0, y1)) return;
    const int gx = (W + TILE - 1) / TILE;
    const unsigned long long zbits = __float_as_uint(zmin[f]);      // zmin > 0.2: the bits of a positive float order as the float does
    long long o = offsets[f];
    const long long stop = o + n;                                    // (never past this face's own rows of the list)
    for (int ty = y0 / TILE; ty <= y1 / TILE; ++ty)
        for (int tx = x0 / TILE; tx <= x1 / TILE && o < stop; ++tx, ++o) {
            keys[o] = ((unsigned long long)(ty * gx + tx) << 32) | zbits;
            vals[o] = (uint32_t)f;
        }
}

__global__ void __launch_bounds__(NT) mesh_tile_ranges_kernel(const unsigned long long* __restrict__ keys, int n, int ntiles,
                                                              int32_t* __restrict__ ranges) {
    const long long il = (long long)blockIdx.x * NT + threadIdx.x;
    if (il >= n) return;
    const int i = (int)il;
    const unsigned tile = (unsigned)(keys[i] >> 32);
    if (tile >= (unsigned)ntiles) return;
    if (i == 0 || (unsigned)(keys[i - 1] >> 32) != tile) ranges[2 * tile] = i;
    if (i == n - 1 || (unsigned)(keys[i + 1] >> 32) != tile) ranges[2 * tile + 1] = i + 1;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Render.  An edge u -> v of a face oriented so that its inside has positive edge functions is a LEFT edge when it runs towards smaller y
// and a TOP edge when it is horizontal and runs towards larger x (y points down): a pixel centre ON such an edge belongs to the face, on
// any other edge it does not.  A face of the other winding has its edge functions negated and its edges reversed first, so two faces that
// share an edge run it in opposite directions whatever their windings, and exactly one of them owns the centres on it.
__device__ __forceinline__ int edge_threshold(int dx, int dy) { return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1; }      // covered: E >= this

__global__ void __launch_bounds__(NT) mesh_render_kernel(const int32_t* __restrict__ ranges, const uint32_t* __restrict__ fid,
                                                         const int32_t* __restrict__ faces, const int32_t* __restrict__ pix_q,
                                                         const float* __restrict__ zv, const float* __restrict__ zmin,
                                                         const float* __restrict__ colors, int W, int H, int gx, int bits, float bg0, float bg1,
                                                         float bg2, float* __restrict__ image, float* __restrict__ out_depth,
                                                         float* __restrict__ out_alpha, int32_t* __restrict__ out_face,
                                                         int32_t* __restrict__ n_hit) {
    __shared__ int4 s_ab[NT];        // ax ay bx by
    __shared__ int4 s_cf[NT];        // cx cy face flags (bits 0 .. 2: thresholds of the edge functions E0 E1 E2, bit 3: negative area)
    __shared__ float4 s_z[NT];       // zv of a b c, zmin
    const int tile = blockIdx.x, t = threadIdx.x;
    const int px = (tile % gx) * TILE + (t % TILE), py = (tile / gx) * TILE + (t / TILE);
    const bool inside = px < W && py < H;
    const int Px = px << bits, Py = py << bits;         // <= 4095 * 256
    const int start = ranges[2 * tile], end = ranges[2 * tile + 1];
    const bool early = n_hit == nullptr;                // (uniform over the grid)
    float best_z = __int_as_float(0x7f800000);
    int best_f = -1, hits = 0;
    float bb0 = 0.f, bb1 = 0.f, bb2 = 0.f;
    for (int base = start; base < end; base += NT) {
        if (early) {
            // the list is ordered by zmin and no face is nearer than its zmin anywhere: once every pixel holds a depth in front of this
            // batch's first zmin nothing behind can win.  (Strictly in front: at equal depth a later entry with a lower face index would.)
            const float zfirst = zmin[fid[base]];
            if (__syncthreads_and(!inside || (best_f >= 0 && best_z < zfirst))) break;
        } else {
            __syncthreads();
        }
        if (base + t < end) {
            const int f = (int)fid[base + t];
            const int i0 = faces[3 * (long long)f], i1 = faces[3 * (long long)f + 1], i2 = faces[3 * (long long)f + 2];
            const int ax = pix_q[2 * (long long)i0], ay = pix_q[2 * (long long)i0 + 1];
            const int bx = pix_q[2 * (long long)i1], by = pix_q[2 * (long long)i1 + 1];
            const int cx = pix_q[2 * (long long)i2], cy = pix_q[2 * (long long)i2 + 1];
            const long long a2 = (long long)(bx - ax) * (cy - ay) - (long long)(by - ay) * (cx - ax);
            const int s = a2 < 0 ? -1 : 1;
            const int flags = edge_threshold(s * (cx - bx), s * (cy - by)) | (edge_threshold(s * (ax - cx), s * (ay - cy)) << 1) |
                              (edge_threshold(s * (bx - ax), s * (by - ay)) << 2) | (a2 < 0 ? 8 : 0);
            s_ab[t] = make_int4(ax, ay, bx, by);
            s_cf[t] = make_int4(cx, cy, f, flags);
            s_z[t] = make_float4(zv[i0], zv[i1], zv[i2], zmin[f]);
        }
        __syncthreads();
        const int cnt = min(NT, end - base);
        for (int j = 0; j < cnt; ++j) {
            const int4 ab = s_ab[j], cf = s_cf[j];
            // E0 = edge b -> c (the weight of a), E1 = edge c -> a, E2 = edge a -> b, at the pixel centre
            long long e0 = (long long)(cf.x - ab.z) * (Py - ab.w) - (long long)(cf.y - ab.w) * (Px - ab.z);
            long long e1 = (long long)(ab.x - cf.x) * (Py - cf.y) - (long long)(ab.y - cf.y) * (Px - cf.x);
            long long e2 = (long long)(ab.z - ab.x) * (Py - ab.y) - (long long)(ab.w - ab.y) * (Px - ab.x);
            if (cf.w & 8) {
                e0 = -e0;
                e1 = -e1;
                e2 = -e2;
            }
            if (e0 < (cf.w & 1) || e1 < ((cf.w >> 1) & 1) || e2 < ((cf.w >> 2) & 1)) continue;
            ++hits;
            const float4 z4 = s_z[j];
            const float fa = (float)(e0 + e1 + e2);
            const float b0 = (float)e0 / fa, b1 = (float)e1 / fa, b2 = (float)e2 / fa;
            float z = 1.f / (b0 / z4.x + b1 / z4.y + b2 / z4.z);
            z = fminf(fmaxf(z, z4.w), fmaxf(z4.x, fmaxf(z4.y, z4.z)));      // a face is nowhere nearer than its zmin nor farther than its zmax
            if (z < best_z || (z == best_z && cf.z < best_f)) {
                best_z = z;
                best_f = cf.z;
                bb0 = b0;
                bb1 = b1;
                bb2 = b2;
            }
        }
    }
    if (!inside) return;
    const long long pix = (long long)py * W + px, HW = (long long)H * W;
    float c0 = bg0, c1 = bg1, c2 = bg2;
    if (best_f >= 0) {
        const int i0 = faces[3 * (long long)best_f], i1 = faces[3 * (long long)best_f + 1], i2 = faces[3 * (long long)best_f + 2];
        const float w0 = bb0 / zv[i0], w1 = bb1 / zv[i1], w2 = bb2 / zv[i2];
        c0 = best_z * (w0 * colors[3 * (long long)i0] + w1 * colors[3 * (long long)i1] + w2 * colors[3 * (long long)i2]);
        c1 = best_z * (w0 * colors[3 * (long long)i0 + 1] + w1 * colors[3 * (long long)i1 + 1] + w2 * colors[3 * (long long)i2 + 1]);
        c2 = best_z * (w0 * colors[3 * (long long)i0 + 2] + w1 * colors[3 * (long long)i1 + 2] + w2 * colors[3 * (long long)i2 + 2]);
    }
    image[pix] = c0;
    image[HW + pix] = c1;
    image[2 * HW + pix] = c2;
    out_depth[pix] = best_f >= 0 ? best_z : 0.f;
    out_alpha[pix] = best_f >= 0 ? 1.f : 0.f;
    out_face[pix] = best_f;
    if (n_hit) n_hit[pix] = hits;
}

bool image_ok(int32_t w, int32_t h) { return w > 0 && h > 0 && w <= V3D_RECON_MESH_MAX_IMAGE && h <= V3D_RECON_MESH_MAX_IMAGE; }
bool bits_ok(int32_t b) { return b >= 0 && b <= V3D_RECON_MESH_MAX_SUBPIXEL_BITS; }

}  // namespace

#define ST ((hipStream_t)stream)
#define MESH_REQUIRE_IMAGE(name, w, h) \
    RECON_REQUIRE(image_ok(w, h), name ": image %d x %d outside 1 .. %d on a side", (int)(w), (int)(h), V3D_RECON_MESH_MAX_IMAGE)
#define MESH_REQUIRE_BITS(name, b) \
    RECON_REQUIRE(bits_ok(b), name ": subpixel_bits %d outside 0 .. %d", (int)(b), V3D_RECON_MESH_MAX_SUBPIXEL_BITS)

extern "C" int v3d_recon_mesh_project(const float* verts, int32_t num_verts, const v3d_gs_camera* cam, int32_t subpixel_bits, float* zv, float* pix_f,
                                      int32_t* pix_q, v3d_stream_t stream) {
    RECON_REQUIRE(verts && cam && zv && pix_f && pix_q, "v3d_recon_mesh_project: null argument");
    RECON_REQUIRE(num_verts > 0, "v3d_recon_mesh_project: num_verts must be positive");
    MESH_REQUIRE_BITS("v3d_recon_mesh_project", subpixel_bits);
    MESH_REQUIRE_IMAGE("v3d_recon_mesh_project", cam->width, cam->height);
    hipLaunchKernelGGL(mesh_project_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, verts, (int)num_verts, *cam, (int)subpixel_bits, zv, pix_f, pix_q);
    return check_launch("v3d_recon_mesh_project");
}

extern "C" int v3d_recon_mesh_face_setup(const int32_t* faces, int32_t num_faces, const int32_t* pix_q, const float* zv, int32_t num_verts,
                                         int32_t width, int32_t height, int32_t subpixel_bits, int32_t cull, int32_t* tiles_touched, float* zmin,
                                         v3d_stream_t stream) {
    RECON_REQUIRE(faces && pix_q && zv && tiles_touched && zmin, "v3d_recon_mesh_face_setup: null argument");
    RECON_REQUIRE(num_faces > 0 && num_verts > 0, "v3d_recon_mesh_face_setup: num_faces and num_verts must be positive");
    MESH_REQUIRE_BITS("v3d_recon_mesh_face_setup", subpixel_bits);
    MESH_REQUIRE_IMAGE("v3d_recon_mesh_face_setup", width, height);
    hipLaunchKernelGGL(mesh_face_setup_kernel, dim3(nblk(num_faces)), dim3(NT), 0, ST, faces, (int)num_faces, pix_q, zv, (int)num_verts, (int)width,
                       (int)height, (int)subpixel_bits, cull ? 1 : 0, tiles_touched, zmin);
    return check_launch("v3d_recon_mesh_face_setup");
}

extern "C" int v3d_recon_mesh_duplicate_keys(const int32_t* faces, int32_t num_faces, const int32_t* pix_q, int32_t num_verts,
                                             const int32_t* tiles_touched, const int32_t* offsets, const float* zmin, int32_t width, int32_t height,
                                             int32_t subpixel_bits, uint64_t* keys, uint32_t* vals, v3d_stream_t stream) {
    RECON_REQUIRE(faces && pix_q && tiles_touched && offsets && zmin && keys && vals, "v3d_recon_mesh_duplicate_keys: null argument");
    RECON_REQUIRE(num_faces > 0 && num_verts > 0, "v3d_recon_mesh_duplicate_keys: num_faces and num_verts must be positive");
    MESH_REQUIRE_BITS("v3d_recon_mesh_duplicate_keys", subpixel_bits);
    MESH_REQUIRE_IMAGE("v3d_recon_mesh_duplicate_keys", width, height);
    hipLaunchKernelGGL(mesh_duplicate_keys_kernel, dim3(nblk(num_faces)), dim3(NT), 0, ST, faces, (int)num_faces, pix_q, (int)num_verts, tiles_touched,
                       offsets, zmin, (int)width, (int)height, (int)subpixel_bits, (unsigned long long*)keys, vals);
    return check_launch("v3d_recon_mesh_duplicate_keys");
}

extern "C" int v3d_recon_mesh_tile_ranges(const uint64_t* keys_sorted, int32_t num_instances, int32_t width, int32_t height, int32_t* ranges,
                                          v3d_stream_t stream) {
    RECON_REQUIRE(ranges && (keys_sorted || num_instances == 0), "v3d_recon_mesh_tile_ranges: null argument");
    RECON_REQUIRE(num_instances >= 0, "v3d_recon_mesh_tile_ranges: num_instances must not be negative");
    MESH_REQUIRE_IMAGE("v3d_recon_mesh_tile_ranges", width, height);
    const int ntiles = ((width + TILE - 1) / TILE) * ((height + TILE - 1) / TILE);
    hipError_t e = hipMemsetAsync(ranges, 0, sizeof(int32_t) * 2 * (size_t)ntiles, ST);
    if (e != hipSuccess) {
        set_error("v3d_recon_mesh_tile_ranges: clearing the ranges failed: %s", hipGetErrorString(e));
        return RC_LAUNCH;
    }
    if (num_instances == 0) return RC_OK;
    hipLaunchKernelGGL(mesh_tile_ranges_kernel, dim3(nblk(num_instances)), dim3(NT), 0, ST, (const unsigned long long*)keys_sorted, (int)num_instances,
                       ntiles, ranges);
    return check_launch("v3d_recon_mesh_tile_ranges");
}

extern "C" int v3d_recon_mesh_render(const int32_t* ranges, const uint32_t* vals_sorted, const int32_t* faces, int32_t num_faces, const int32_t* pix_q,
                                     const float* zv, const float* zmin, const float* colors, const v3d_gs_camera* cam, int32_t subpixel_bits,
                                     float* image, float* depth, float* alpha, int32_t* face_id, int32_t* n_hit, v3d_stream_t stream) {
    RECON_REQUIRE(ranges && faces && pix_q && zv && zmin && colors && cam && image && depth && alpha && face_id,
                  "v3d_recon_mesh_render: null argument");
    RECON_REQUIRE(num_faces > 0, "v3d_recon_mesh_render: num_faces must be positive");
    MESH_REQUIRE_BITS("v3d_recon_mesh_render", subpixel_bits);
    MESH_REQUIRE_IMAGE("v3d_recon_mesh_render", cam->width, cam->height);
    const int W = cam->width, H = cam->height;
    const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
    hipLaunchKernelGGL(mesh_render_kernel, dim3(gx * gy), dim3(NT), 0, ST, ranges, vals_sorted, faces, pix_q, zv, zmin, colors, W, H, gx,
                       (int)subpixel_bits, cam->bg[0], cam->bg[1], cam->bg[2], image, depth, alpha, face_id, n_hit);
    return check_launch("v3d_recon_mesh_render");
}
