// Vertex-colour refinement of the extracted mesh (include/v3d_recon.h "Mesh colour refinement", libv3d_recon.so; host side:
// v3d_amd/recon/mesh_refine.py).  The geometry is fixed, so what a camera sees never changes: the forward of meshrast.hip runs once per view
// and its face_id map is frozen here into three vertex indices and three weights per pixel (pixel_weights).  The image is then a fixed sparse
// linear map of the vertex colours (shade: a gather per pixel) and the gradient with respect to the colours is its transpose (shade_bwd: a
// gather per vertex over a list that vertex_records -> v3d_gs_radix_sort_pairs -> vertex_ranges built once).  color_adam is the optimiser's
// step on the colours' logits.  The scan and the sort are libv3d_hip.so's, called by the host.
//
// No atomics: a pixel, a record and an element each belong to one thread, a vertex to one wave, which sums its list in a fixed order.
// Built without -ffast-math (v3d_amd/build.py): everything is held to an fp64 restatement (tests/mesh_refine_ref.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "recon_host.h"
#include "v3d_recon.h"

namespace {

constexpr int WAVE = 64;

// ---------------------------------------------------------------------------------------------------------------------------------------
// Per-pixel vertices and weights.  The edge functions, the orientation flip and the quotients are mesh_render_kernel's (meshrast.hip),
// statement for statement, on the face that won the pixel there.
__global__ void __launch_bounds__(NT) mesh_pixel_weights_kernel(const int32_t* __restrict__ face_id, const int32_t* __restrict__ faces, int nf,
                                                                const int32_t* __restrict__ pix_q, const float* __restrict__ zv, int nv, int W,
                                                                int H, int bits, int32_t* __restrict__ pix_vert, float* __restrict__ pix_w) {
    const long long pix = (long long)blockIdx.x * NT + threadIdx.x;
    if (pix >= (long long)W * H) return;
    int v0 = -1, v1 = -1, v2 = -1;
    float w0 = 0.f, w1 = 0.f, w2 = 0.f;
    const int f = face_id[pix];
    if (f >= 0 && f < nf) {
        const int i0 = faces[3 * (long long)f], i1 = faces[3 * (long long)f + 1], i2 = faces[3 * (long long)f + 2];
        if (i0 >= 0 && i0 < nv && i1 >= 0 && i1 < nv && i2 >= 0 && i2 < nv) {      // (always, on a face the forward drew)
            const int Px = (int)(pix % W) << bits, Py = (int)(pix / W) << bits;
            const int ax = pix_q[2 * (long long)i0], ay = pix_q[2 * (long long)i0 + 1];
            const int bx = pix_q[2 * (long long)i1], by = pix_q[2 * (long long)i1 + 1];
            const int cx = pix_q[2 * (long long)i2], cy = pix_q[2 * (long long)i2 + 1];
            const long long a2 = (long long)(bx - ax) * (cy - ay) - (long long)(by - ay) * (cx - ax);
            // E0 = edge b -> c (the weight of a), E1 = edge c -> a, E2 = edge a -> b, at the pixel centre
            long long e0 = (long long)(cx - bx) * (Py - by) - (long long)(cy - by) * (Px - bx);
            long long e1 = (long long)(ax - cx) * (Py - cy) - (long long)(ay - cy) * (Px - cx);
            long long e2 = (long long)(bx - ax) * (Py - ay) - (long long)(by - ay) * (Px - ax);
            if (a2 < 0) {
                e0 = -e0;
                e1 = -e1;
                e2 = -e2;
            }
            const float fa = (float)(e0 + e1 + e2);
            const float b0 = (float)e0 / fa, b1 = (float)e1 / fa, b2 = (float)e2 / fa;
            v0 = i0, v1 = i1, v2 = i2;
            w0 = b0 / zv[i0], w1 = b1 / zv[i1], w2 = b2 / zv[i2];
        }
    }
    pix_vert[3 * pix] = v0;
    pix_vert[3 * pix + 1] = v1;
    pix_vert[3 * pix + 2] = v2;
    pix_w[3 * pix] = w0;
    pix_w[3 * pix + 1] = w1;
    pix_w[3 * pix + 2] = w2;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Shade: the statement mesh_render_kernel shades its winner with.
__global__ void __launch_bounds__(NT) mesh_shade_kernel(const int32_t* __restrict__ pix_vert, const float* __restrict__ pix_w,
                                                        const float* __restrict__ depth, const float* __restrict__ colors, int nv, long long HW,
                                                        float bg0, float bg1, float bg2, float* __restrict__ image) {
    const long long pix = (long long)blockIdx.x * NT + threadIdx.x;
    if (pix >= HW) return;
    const int i0 = pix_vert[3 * pix], i1 = pix_vert[3 * pix + 1], i2 = pix_vert[3 * pix + 2];
    float c0 = bg0, c1 = bg1, c2 = bg2;
    if (i0 >= 0 && i0 < nv && i1 >= 0 && i1 < nv && i2 >= 0 && i2 < nv) {
        const float w0 = pix_w[3 * pix], w1 = pix_w[3 * pix + 1], w2 = pix_w[3 * pix + 2];
        const float best_z = depth[pix];
        c0 = best_z * (w0 * colors[3 * (long long)i0] + w1 * colors[3 * (long long)i1] + w2 * colors[3 * (long long)i2]);
        c1 = best_z * (w0 * colors[3 * (long long)i0 + 1] + w1 * colors[3 * (long long)i1 + 1] + w2 * colors[3 * (long long)i2 + 1]);
        c2 = best_z * (w0 * colors[3 * (long long)i0 + 2] + w1 * colors[3 * (long long)i1 + 2] + w2 * colors[3 * (long long)i2 + 2]);
    }
    image[pix] = c0;
    image[HW + pix] = c1;
    image[2 * HW + pix] = c2;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The transposed lists.  Three records per covered pixel at rows 3 offsets[pixel] .. + 2, in pixel order: the stable sort on the vertex then
// leaves every vertex's records in ascending 3 pixel + k.
__global__ void __launch_bounds__(NT) mesh_vertex_records_kernel(const int32_t* __restrict__ pix_vert, const int32_t* __restrict__ offsets,
                                                                 long long HW, int n, unsigned long long* __restrict__ keys,
                                                                 uint32_t* __restrict__ vals) {
    const long long pix = (long long)blockIdx.x * NT + threadIdx.x;
    if (pix >= HW) return;
    if (pix_vert[3 * pix] < 0) return;
    const long long o = 3 * (long long)offsets[pix];
    if (o < 0 || o + 3 > n) return;                                  // (never, with the offsets of this coverage)
    for (int k = 0; k < 3; ++k) {
        keys[o + k] = (unsigned long long)(uint32_t)pix_vert[3 * pix + k];
        vals[o + k] = (uint32_t)(3 * pix + k);
    }
}

__global__ void __launch_bounds__(NT) mesh_vertex_ranges_kernel(const unsigned long long* __restrict__ keys, int n, int nv,
                                                                int32_t* __restrict__ ranges) {
    const long long il = (long long)blockIdx.x * NT + threadIdx.x;
    if (il >= n) return;
    const int i = (int)il;
    const unsigned long long v = keys[i];
    if (v >= (unsigned long long)nv) return;
    if (i == 0 || keys[i - 1] != v) ranges[2 * v] = i;
    if (i == n - 1 || keys[i + 1] != v) ranges[2 * v + 1] = i + 1;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The transpose.  One wave per vertex: lane l adds entries start + l, start + l + 64, .. in that order, then the 64 partial sums meet in the
// xor butterfly of v3d_gs_render_bwd.  The order depends on the list alone, not on the launch.
__global__ void __launch_bounds__(NT) mesh_shade_bwd_kernel(const int32_t* __restrict__ ranges, const int32_t* __restrict__ ent_pix,
                                                            const float* __restrict__ ent_w, int n, const float* __restrict__ dL_dimage,
                                                            long long HW, int nv, float* __restrict__ dL_dcolors) {
    const long long vl = (long long)blockIdx.x * (NT / WAVE) + threadIdx.x / WAVE;       // (uniform over the wave)
    if (vl >= nv) return;
    const int lane = threadIdx.x % WAVE;
    const int start = max(ranges[2 * vl], 0), end = min(ranges[2 * vl + 1], n);
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    for (int i = start + lane; i < end; i += WAVE) {
        const long long p = ent_pix[i];
        if (p < 0 || p >= HW) continue;
        const float w = ent_w[i];
        g0 += w * dL_dimage[p];
        g1 += w * dL_dimage[HW + p];
        g2 += w * dL_dimage[2 * HW + p];
    }
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        g0 += __shfl_xor(g0, o, WAVE);
        g1 += __shfl_xor(g1, o, WAVE);
        g2 += __shfl_xor(g2, o, WAVE);
    }
    if (lane == 0) {
        dL_dcolors[3 * vl] = g0;
        dL_dcolors[3 * vl + 1] = g1;
        dL_dcolors[3 * vl + 2] = g2;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Adam on the logits: the statements of torch.optim.Adam (lerp of the first moment, bias corrections, eps outside the square root).
__global__ void __launch_bounds__(NT) mesh_color_adam_kernel(float* __restrict__ logit, float* __restrict__ m, float* __restrict__ v,
                                                             const float* __restrict__ grad, long long n, float one_minus_beta1, float beta2,
                                                             float one_minus_beta2, float step_size, float bc2_sqrt, float eps,
                                                             float* __restrict__ colors) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    float x = logit[i];
    const float s = 1.f / (1.f + expf(-x));
    const float g = grad[i] * s * (1.f - s);
    float mi = m[i], vi = v[i];
    mi = mi + (g - mi) * one_minus_beta1;
    vi = vi * beta2 + one_minus_beta2 * g * g;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    x = x - step_size * (mi / denom);                   // g == 0 on every step so far: m == 0, and x - 0 is x
    m[i] = mi;
    v[i] = vi;
    logit[i] = x;
    colors[i] = 1.f / (1.f + expf(-x));
}

bool image_ok(int32_t w, int32_t h) { return w > 0 && h > 0 && w <= V3D_RECON_MESH_MAX_IMAGE && h <= V3D_RECON_MESH_MAX_IMAGE; }

}  // namespace

#define ST ((hipStream_t)stream)
#define SHADE_REQUIRE_IMAGE(name, w, h) \
    RECON_REQUIRE(image_ok(w, h), name ": image %d x %d outside 1 .. %d on a side", (int)(w), (int)(h), V3D_RECON_MESH_MAX_IMAGE)

extern "C" int v3d_recon_mesh_pixel_weights(const int32_t* face_id, const int32_t* faces, int32_t num_faces, const int32_t* pix_q, const float* zv,
                                            int32_t num_verts, int32_t width, int32_t height, int32_t subpixel_bits, int32_t* pix_vert, float* pix_w,
                                            v3d_stream_t stream) {
    RECON_REQUIRE(face_id && faces && pix_q && zv && pix_vert && pix_w, "v3d_recon_mesh_pixel_weights: null argument");
    RECON_REQUIRE(num_faces > 0 && num_verts > 0, "v3d_recon_mesh_pixel_weights: num_faces and num_verts must be positive");
    RECON_REQUIRE(subpixel_bits >= 0 && subpixel_bits <= V3D_RECON_MESH_MAX_SUBPIXEL_BITS, "v3d_recon_mesh_pixel_weights: subpixel_bits %d outside 0 .. %d",
                  (int)subpixel_bits, V3D_RECON_MESH_MAX_SUBPIXEL_BITS);
    SHADE_REQUIRE_IMAGE("v3d_recon_mesh_pixel_weights", width, height);
    hipLaunchKernelGGL(mesh_pixel_weights_kernel, dim3(nblk((long long)width * height)), dim3(NT), 0, ST, face_id, faces, (int)num_faces, pix_q, zv,
                       (int)num_verts, (int)width, (int)height, (int)subpixel_bits, pix_vert, pix_w);
    return check_launch("v3d_recon_mesh_pixel_weights");
}

extern "C" int v3d_recon_mesh_shade(const int32_t* pix_vert, const float* pix_w, const float* depth, const float* colors, int32_t num_verts,
                                    int32_t width, int32_t height, float bg0, float bg1, float bg2, float* image, v3d_stream_t stream) {
    RECON_REQUIRE(pix_vert && pix_w && depth && colors && image, "v3d_recon_mesh_shade: null argument");
    RECON_REQUIRE(num_verts > 0, "v3d_recon_mesh_shade: num_verts must be positive");
    SHADE_REQUIRE_IMAGE("v3d_recon_mesh_shade", width, height);
    const long long HW = (long long)width * height;
    hipLaunchKernelGGL(mesh_shade_kernel, dim3(nblk(HW)), dim3(NT), 0, ST, pix_vert, pix_w, depth, colors, (int)num_verts, HW, bg0, bg1, bg2, image);
    return check_launch("v3d_recon_mesh_shade");
}

extern "C" int v3d_recon_mesh_vertex_records(const int32_t* pix_vert, const int32_t* offsets, int32_t width, int32_t height, int32_t num_records,
                                             uint64_t* keys, uint32_t* vals, v3d_stream_t stream) {
    RECON_REQUIRE(pix_vert && offsets && keys && vals, "v3d_recon_mesh_vertex_records: null argument");
    SHADE_REQUIRE_IMAGE("v3d_recon_mesh_vertex_records", width, height);
    const long long HW = (long long)width * height;
    RECON_REQUIRE(num_records > 0 && num_records % 3 == 0 && num_records <= 3 * HW,
                  "v3d_recon_mesh_vertex_records: num_records %d is not a positive multiple of 3 up to 3 x the pixel count", (int)num_records);
    hipLaunchKernelGGL(mesh_vertex_records_kernel, dim3(nblk(HW)), dim3(NT), 0, ST, pix_vert, offsets, HW, (int)num_records, (unsigned long long*)keys,
                       vals);
    return check_launch("v3d_recon_mesh_vertex_records");
}

extern "C" int v3d_recon_mesh_vertex_ranges(const uint64_t* keys_sorted, int32_t num_records, int32_t num_verts, int32_t* ranges,
                                            v3d_stream_t stream) {
    RECON_REQUIRE(ranges && (keys_sorted || num_records == 0), "v3d_recon_mesh_vertex_ranges: null argument");
    RECON_REQUIRE(num_records >= 0, "v3d_recon_mesh_vertex_ranges: num_records must not be negative");
    RECON_REQUIRE(num_verts > 0, "v3d_recon_mesh_vertex_ranges: num_verts must be positive");
    hipError_t e = hipMemsetAsync(ranges, 0, sizeof(int32_t) * 2 * (size_t)num_verts, ST);
    if (e != hipSuccess) {
        set_error("v3d_recon_mesh_vertex_ranges: clearing the ranges failed: %s", hipGetErrorString(e));
        return RC_LAUNCH;
    }
    if (num_records == 0) return RC_OK;
    hipLaunchKernelGGL(mesh_vertex_ranges_kernel, dim3(nblk(num_records)), dim3(NT), 0, ST, (const unsigned long long*)keys_sorted, (int)num_records,
                       (int)num_verts, ranges);
    return check_launch("v3d_recon_mesh_vertex_ranges");
}

extern "C" int v3d_recon_mesh_shade_bwd(const int32_t* ranges, const int32_t* ent_pix, const float* ent_w, int32_t num_entries, const float* dL_dimage,
                                        int32_t width, int32_t height, int32_t num_verts, float* dL_dcolors, v3d_stream_t stream) {
    RECON_REQUIRE(ranges && dL_dimage && dL_dcolors && ((ent_pix && ent_w) || num_entries == 0), "v3d_recon_mesh_shade_bwd: null argument");
    RECON_REQUIRE(num_entries >= 0, "v3d_recon_mesh_shade_bwd: num_entries must not be negative");
    RECON_REQUIRE(num_verts > 0, "v3d_recon_mesh_shade_bwd: num_verts must be positive");
    SHADE_REQUIRE_IMAGE("v3d_recon_mesh_shade_bwd", width, height);
    const long long blocks = ((long long)num_verts + NT / WAVE - 1) / (NT / WAVE);
    hipLaunchKernelGGL(mesh_shade_bwd_kernel, dim3((unsigned)blocks), dim3(NT), 0, ST, ranges, ent_pix, ent_w, (int)num_entries, dL_dimage,
                       (long long)width * height, (int)num_verts, dL_dcolors);
    return check_launch("v3d_recon_mesh_shade_bwd");
}

extern "C" int v3d_recon_mesh_color_adam(float* logit, float* m, float* v, const float* grad, int32_t num_verts, double lr, double beta1, double beta2,
                                         double eps, int32_t step, float* colors, v3d_stream_t stream) {
    RECON_REQUIRE(logit && m && v && grad && colors, "v3d_recon_mesh_color_adam: null argument");
    RECON_REQUIRE(num_verts > 0, "v3d_recon_mesh_color_adam: num_verts must be positive");
    RECON_REQUIRE(step >= 1, "v3d_recon_mesh_color_adam: step %d must be 1 or more", (int)step);
    RECON_REQUIRE(lr >= 0.0 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps > 0.0,        // (false on NaN)
                  "v3d_recon_mesh_color_adam: lr %g, betas %g %g, eps %g outside lr >= 0, 0 <= beta < 1, eps > 0", lr, beta1, beta2, eps);
    // the scalars in double on the host, as torch.optim.Adam computes them, rounded to fp32 once
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    hipLaunchKernelGGL(mesh_color_adam_kernel, dim3(nblk(3LL * num_verts)), dim3(NT), 0, ST, logit, m, v, grad, 3LL * num_verts, (float)(1.0 - beta1),
                       (float)beta2, (float)(1.0 - beta2), (float)(lr / bc1), (float)sqrt(bc2), (float)eps, colors);
    return check_launch("v3d_recon_mesh_color_adam");
}
