// Silhouette fit of the mesh's vertices (include/v3d_recon.h "Mesh vertex fit", libv3d_recon.so; host side: v3d_amd/recon/mesh_deform.py).
// The forward of meshrast.hip decides coverage on integers; this file antialiases that coverage at the border between the object and the
// background and carries the gradient of the antialiased alpha to the vertex positions:
//   aa_alpha (one thread per pixel, a gather over its four neighbours)
//   aa_count -> v3d_gs_scan -> aa_emit -> v3d_gs_radix_sort_pairs -> vertex_ranges (meshshade.hip) -> aa_reduce (one wave per vertex)
//   project_bwd (one thread per vertex: dL/dpix_f through the statements of mesh_project_kernel to dL/dverts)
//   smooth_grad (one thread per vertex over the corner lists of meshtopo.hip: the gradient of the deformation field's edge energy)
// The scan and the sort are libv3d_hip.so's, called by the host.
//
// No atomics: a pixel, a record and a vertex row each belong to one thread, a vertex's list to one wave, which sums it in a fixed order.
// The pair rule is evaluated by ONE device function with explicitly rounded products (no contraction into fused multiply-adds), so the
// three kernels that walk the pairs take the same decisions bit for bit.  Built without -ffast-math (v3d_amd/build.py): everything is held
// to an fp64 restatement (tests/mesh_deform_ref.py).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "recon_host.h"
#include "v3d_recon.h"

namespace {

constexpr int WAVE = 64;
constexpr int MARK = INT32_MIN;

// ---------------------------------------------------------------------------------------------------------------------------------------
// The pair rule.  A pair is a covered pixel p (face f) and a neighbour q inside the image that nothing covers.
struct AaFace {
    int i[3];
    float x[3], y[3];
    float s;          // -1 where the doubled area of the SNAPPED corners is negative (the rasterizer's own integer decision), else +1
};

__device__ __forceinline__ bool aa_face(const int32_t* __restrict__ faces, int nf, const float* __restrict__ pix_f,
                                        const int32_t* __restrict__ pix_q, int nv, int f, AaFace& a) {
    if (f < 0 || f >= nf) return false;
    int qx[3], qy[3];
    for (int k = 0; k < 3; ++k) {
        a.i[k] = faces[3 * (long long)f + k];
        if (a.i[k] < 0 || a.i[k] >= nv) return false;
        qx[k] = pix_q[2 * (long long)a.i[k]];
        qy[k] = pix_q[2 * (long long)a.i[k] + 1];
        if (qx[k] == MARK || qy[k] == MARK) return false;      // (never, on a face the forward drew)
        a.x[k] = pix_f[2 * (long long)a.i[k]];
        a.y[k] = pix_f[2 * (long long)a.i[k] + 1];
    }
    const long long a2 = (long long)(qx[1] - qx[0]) * (qy[2] - qy[0]) - (long long)(qy[1] - qy[0]) * (qx[2] - qx[0]);
    a.s = a2 < 0 ? -1.f : 1.f;
    return true;
}

// E_k(x) = s cross(v - u, x - u) of the edge corner k -> corner k + 1: every product and difference rounded on its own
__device__ __forceinline__ float aa_edge(const AaFace& a, int k, float X, float Y) {
    const int k1 = k == 2 ? 0 : k + 1;
    const float dx = __fsub_rn(a.x[k1], a.x[k]), dy = __fsub_rn(a.y[k1], a.y[k]);
    const float rx = __fsub_rn(X, a.x[k]), ry = __fsub_rn(Y, a.y[k]);
    return __fmul_rn(a.s, __fsub_rn(__fmul_rn(dx, ry), __fmul_rn(dy, rx)));
}

struct AaPair {
    int k;            // the chosen edge, -1 without a candidate
    float t, ep, eq;  // ep: E_k(p) before the clamp at 0
};

__device__ __forceinline__ AaPair aa_pair(const AaFace& a, float px, float py, float qx, float qy) {
    AaPair r;
    r.k = -1;
    r.t = 0.f;
    r.ep = 0.f;
    r.eq = 0.f;
    for (int k = 0; k < 3; ++k) {
        const float eq = aa_edge(a, k, qx, qy);
        if (!(eq < 0.f)) continue;
        const float e = aa_edge(a, k, px, py);
        const float ep = fmaxf(e, 0.f);
        const float t = __fdiv_rn(ep, __fsub_rn(ep, eq));
        if (r.k < 0 || t < r.t) {      // on equal t the lower k stays
            r.k = k;
            r.t = t;
            r.ep = e;
            r.eq = eq;
        }
    }
    return r;
}

// neighbours in the order right, left, down, up
__device__ __forceinline__ void aa_neighbour(int j, int x, int y, int& nx, int& ny) {
    nx = x + (j == 0 ? 1 : (j == 1 ? -1 : 0));
    ny = y + (j == 2 ? 1 : (j == 3 ? -1 : 0));
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Forward: a gather.  A covered pixel adds t - 0.5 of its pairs with t < 0.5 to its 1; a background pixel adds t - 0.5 of the pairs of its
// covered neighbours with t >= 0.5 to its 0: both in the pixel's own neighbour order.
__global__ void __launch_bounds__(NT) mesh_aa_alpha_kernel(const int32_t* __restrict__ face_id, const int32_t* __restrict__ faces, int nf,
                                                           const float* __restrict__ pix_f, const int32_t* __restrict__ pix_q, int nv, int W, int H,
                                                           float* __restrict__ alpha_aa, float* __restrict__ alpha_raw) {
    const long long pix = (long long)blockIdx.x * NT + threadIdx.x;
    if (pix >= (long long)W * H) return;
    const int x = (int)(pix % W), y = (int)(pix / W);
    const int f = face_id[pix];
    float sum = f >= 0 ? 1.f : 0.f;
    AaFace a;
    const bool mine = f >= 0 && aa_face(faces, nf, pix_f, pix_q, nv, f, a);
    for (int j = 0; j < 4; ++j) {
        int nx, ny;
        aa_neighbour(j, x, y, nx, ny);
        if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;
        const int g = face_id[(long long)ny * W + nx];
        if (f >= 0) {
            if (g >= 0 || !mine) continue;
            const AaPair r = aa_pair(a, (float)x, (float)y, (float)nx, (float)ny);
            if (r.k >= 0 && r.t < 0.5f) sum += r.t - 0.5f;
        } else {
            if (g < 0 || !aa_face(faces, nf, pix_f, pix_q, nv, g, a)) continue;
            const AaPair r = aa_pair(a, (float)nx, (float)ny, (float)x, (float)y);
            if (r.k >= 0 && !(r.t < 0.5f)) sum += r.t - 0.5f;
        }
    }
    alpha_raw[pix] = sum;
    alpha_aa[pix] = fminf(fmaxf(sum, 0.f), 1.f);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Count: two records per pair with a candidate, per covered pixel.  pair_info [H][W][4] (optional): per neighbour -1 where there is no
// pair, -2 for a pair without a candidate, else the chosen edge k, + 4 when the receiver is the neighbour.
__global__ void __launch_bounds__(NT) mesh_aa_count_kernel(const int32_t* __restrict__ face_id, const int32_t* __restrict__ faces, int nf,
                                                           const float* __restrict__ pix_f, const int32_t* __restrict__ pix_q, int nv, int W, int H,
                                                           int32_t* __restrict__ counts, int32_t* __restrict__ pair_info) {
    const long long pix = (long long)blockIdx.x * NT + threadIdx.x;
    if (pix >= (long long)W * H) return;
    const int x = (int)(pix % W), y = (int)(pix / W);
    const int f = face_id[pix];
    AaFace a;
    const bool mine = f >= 0 && aa_face(faces, nf, pix_f, pix_q, nv, f, a);
    int n = 0;
    for (int j = 0; j < 4; ++j) {
        int nx, ny, info = -1;
        aa_neighbour(j, x, y, nx, ny);
        if (mine && nx >= 0 && nx < W && ny >= 0 && ny < H && face_id[(long long)ny * W + nx] < 0) {
            const AaPair r = aa_pair(a, (float)x, (float)y, (float)nx, (float)ny);
            info = r.k < 0 ? -2 : r.k + (r.t < 0.5f ? 0 : 4);
            if (r.k >= 0) n += 2;
        }
        if (pair_info) pair_info[4 * pix + j] = info;
    }
    counts[pix] = n;
}

// Emit: the records of pixel p at rows offsets[p] .., in neighbour-then-corner order: key = vertex, value = the record's own row, payload =
// dL/dpix_f of that vertex from that pair.  dL/dt is the gradient at the receiver, 0 where the receiver's unclamped sum lies outside the
// open interval (0, 1) or E_k(p) was clamped; t = Ep / (Ep - Eq) then goes to the chosen edge's two corners in closed form.
__global__ void __launch_bounds__(NT) mesh_aa_emit_kernel(const int32_t* __restrict__ face_id, const int32_t* __restrict__ faces, int nf,
                                                          const float* __restrict__ pix_f, const int32_t* __restrict__ pix_q, int nv, int W, int H,
                                                          const float* __restrict__ alpha_raw, const float* __restrict__ dL_dalpha,
                                                          const int32_t* __restrict__ offsets, int n, unsigned long long* __restrict__ keys,
                                                          uint32_t* __restrict__ vals, float* __restrict__ payload) {
    const long long pix = (long long)blockIdx.x * NT + threadIdx.x;
    if (pix >= (long long)W * H) return;
    const int x = (int)(pix % W), y = (int)(pix / W);
    const int f = face_id[pix];
    AaFace a;
    if (f < 0 || !aa_face(faces, nf, pix_f, pix_q, nv, f, a)) return;
    long long o = offsets[pix];
    if (o < 0) return;
    for (int j = 0; j < 4; ++j) {
        int nx, ny;
        aa_neighbour(j, x, y, nx, ny);
        if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;
        const long long qpix = (long long)ny * W + nx;
        if (face_id[qpix] >= 0) continue;
        const float px = (float)x, py = (float)y, qx = (float)nx, qy = (float)ny;
        const AaPair r = aa_pair(a, px, py, qx, qy);
        if (r.k < 0) continue;
        if (o + 2 > n) return;                                   // (never, with the offsets of this coverage)
        const long long rec = r.t < 0.5f ? pix : qpix;
        const float raw = alpha_raw[rec];
        float g = dL_dalpha[rec];
        if (!(raw > 0.f && raw < 1.f) || r.ep < 0.f) g = 0.f;
        const int k = r.k, k1 = k == 2 ? 0 : k + 1;
        const float ep = fmaxf(r.ep, 0.f), den = ep - r.eq;      // > 0: eq < 0 <= ep
        const float gp = g * (-r.eq / (den * den)), gq = g * (ep / (den * den));      // dL/dE(p), dL/dE(q)
        const float ux = a.x[k], uy = a.y[k], vx = a.x[k1], vy = a.y[k1];
        // dE(X)/du = s (vy - Y, X - vx), dE(X)/dv = s (Y - uy, ux - X)
        const float gux = a.s * (gp * (vy - py) + gq * (vy - qy)), guy = a.s * (gp * (px - vx) + gq * (qx - vx));
        const float gvx = a.s * (gp * (py - uy) + gq * (qy - uy)), gvy = a.s * (gp * (ux - px) + gq * (ux - qx));
        keys[o] = (unsigned long long)(uint32_t)a.i[k];
        vals[o] = (uint32_t)o;
        payload[2 * o] = gux;
        payload[2 * o + 1] = guy;
        keys[o + 1] = (unsigned long long)(uint32_t)a.i[k1];
        vals[o + 1] = (uint32_t)(o + 1);
        payload[2 * o + 2] = gvx;
        payload[2 * o + 3] = gvy;
        o += 2;
    }
}

// One wave per vertex: lane l adds entries start + l, start + l + 64, .. in list order, then the xor butterfly of mesh_shade_bwd_kernel.
__global__ void __launch_bounds__(NT) mesh_aa_reduce_kernel(const int32_t* __restrict__ ranges, const uint32_t* __restrict__ vals_sorted,
                                                            const float* __restrict__ payload, int n, int nv, float* __restrict__ dL_dpix) {
    const long long vl = (long long)blockIdx.x * (NT / WAVE) + threadIdx.x / WAVE;       // (uniform over the wave)
    if (vl >= nv) return;
    const int lane = threadIdx.x % WAVE;
    const int start = max(ranges[2 * vl], 0), end = min(ranges[2 * vl + 1], n);
    float g0 = 0.f, g1 = 0.f;
    for (int i = start + lane; i < end; i += WAVE) {
        const uint32_t r = vals_sorted[i];
        if (r >= (uint32_t)n) continue;
        g0 += payload[2 * (long long)r];
        g1 += payload[2 * (long long)r + 1];
    }
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        g0 += __shfl_xor(g0, o, WAVE);
        g1 += __shfl_xor(g1, o, WAVE);
    }
    if (lane == 0) {
        dL_dpix[2 * vl] = g0;
        dL_dpix[2 * vl + 1] = g1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The projection's backward: the statements of mesh_project_kernel (meshrast.hip) differentiated, the 1 / (hw + 1e-7) included.
__global__ void __launch_bounds__(NT) mesh_project_bwd_kernel(const float* __restrict__ verts, int nv, v3d_gs_camera cam,
                                                              const int32_t* __restrict__ pix_q, const float* __restrict__ dL_dpix,
                                                              float* __restrict__ dL_dverts) {
    const long long vl = (long long)blockIdx.x * NT + threadIdx.x;
    if (vl >= nv) return;
    float dx = 0.f, dy = 0.f, dz = 0.f;
    if (pix_q[2 * vl] != MARK && pix_q[2 * vl + 1] != MARK) {
        const float x = verts[3 * vl], y = verts[3 * vl + 1], z = verts[3 * vl + 2];
        const float* P = cam.proj;
        const float hx = x * P[0] + y * P[4] + z * P[8] + P[12];
        const float hy = x * P[1] + y * P[5] + z * P[9] + P[13];
        const float hw = x * P[3] + y * P[7] + z * P[11] + P[15];
        const float pw = 1.f / (hw + 0.0000001f);
        const float gx = dL_dpix[2 * vl] * (0.5f * (float)cam.width), gy = dL_dpix[2 * vl + 1] * (0.5f * (float)cam.height);
        const float ghx = gx * pw, ghy = gy * pw;
        const float ghw = -(gx * hx + gy * hy) * (pw * pw);
        dx = ghx * P[0] + ghy * P[1] + ghw * P[3];
        dy = ghx * P[4] + ghy * P[5] + ghw * P[7];
        dz = ghx * P[8] + ghy * P[9] + ghw * P[11];
    }
    dL_dverts[3 * vl] = dx;
    dL_dverts[3 * vl + 1] = dy;
    dL_dverts[3 * vl + 2] = dz;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The gradient of sum over faces and their 3 edges of |d_a - d_b|^2: per vertex, in corner order, scale x the sum of (2 d_i - d_j - d_k).
__global__ void __launch_bounds__(NT) mesh_smooth_grad_kernel(const float* __restrict__ d, int nv, const int32_t* __restrict__ faces, int nf,
                                                              const int32_t* __restrict__ ranges, const int32_t* __restrict__ corners, float scale,
                                                              float* __restrict__ grad) {
    const long long v = (long long)blockIdx.x * NT + threadIdx.x;
    if (v >= nv) return;
    const int start = max(ranges[2 * v], 0), end = min(ranges[2 * v + 1], 3 * nf);
    const float px = d[3 * v], py = d[3 * v + 1], pz = d[3 * v + 2];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int i = start; i < end; ++i) {
        const int c = corners[i];
        if (c < 0 || c >= 3 * nf) continue;
        const int f = c / 3, k = c % 3;
        const int i0 = faces[3 * (long long)f], i1 = faces[3 * (long long)f + 1], i2 = faces[3 * (long long)f + 2];
        if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) continue;      // an absent face
        const long long a = k == 0 ? i1 : (k == 1 ? i2 : i0), b = k == 0 ? i2 : (k == 1 ? i0 : i1);
        sx += 2.f * px - d[3 * a] - d[3 * b];
        sy += 2.f * py - d[3 * a + 1] - d[3 * b + 1];
        sz += 2.f * pz - d[3 * a + 2] - d[3 * b + 2];
    }
    grad[3 * v] = scale * sx;
    grad[3 * v + 1] = scale * sy;
    grad[3 * v + 2] = scale * sz;
}

bool image_ok(int32_t w, int32_t h) { return w > 0 && h > 0 && w <= V3D_RECON_MESH_MAX_IMAGE && h <= V3D_RECON_MESH_MAX_IMAGE; }

}  // namespace

#define ST ((hipStream_t)stream)
#define AA_REQUIRE_IMAGE(name, w, h) \
    RECON_REQUIRE(image_ok(w, h), name ": image %d x %d outside 1 .. %d on a side", (int)(w), (int)(h), V3D_RECON_MESH_MAX_IMAGE)
#define AA_REQUIRE_MESH(name, nf, nv) \
    RECON_REQUIRE((nf) > 0 && (nv) > 0, name ": num_faces and num_verts must be positive")

extern "C" int v3d_recon_mesh_aa_alpha(const int32_t* face_id, const int32_t* faces, int32_t num_faces, const float* pix_f, const int32_t* pix_q,
                                       int32_t num_verts, int32_t width, int32_t height, float* alpha_aa, float* alpha_raw, v3d_stream_t stream) {
    RECON_REQUIRE(face_id && faces && pix_f && pix_q && alpha_aa && alpha_raw, "v3d_recon_mesh_aa_alpha: null argument");
    AA_REQUIRE_MESH("v3d_recon_mesh_aa_alpha", num_faces, num_verts);
    AA_REQUIRE_IMAGE("v3d_recon_mesh_aa_alpha", width, height);
    hipLaunchKernelGGL(mesh_aa_alpha_kernel, dim3(nblk((long long)width * height)), dim3(NT), 0, ST, face_id, faces, (int)num_faces, pix_f, pix_q,
                       (int)num_verts, (int)width, (int)height, alpha_aa, alpha_raw);
    return check_launch("v3d_recon_mesh_aa_alpha");
}

extern "C" int v3d_recon_mesh_aa_count(const int32_t* face_id, const int32_t* faces, int32_t num_faces, const float* pix_f, const int32_t* pix_q,
                                       int32_t num_verts, int32_t width, int32_t height, int32_t* counts, int32_t* pair_info, v3d_stream_t stream) {
    RECON_REQUIRE(face_id && faces && pix_f && pix_q && counts, "v3d_recon_mesh_aa_count: null argument");
    AA_REQUIRE_MESH("v3d_recon_mesh_aa_count", num_faces, num_verts);
    AA_REQUIRE_IMAGE("v3d_recon_mesh_aa_count", width, height);
    hipLaunchKernelGGL(mesh_aa_count_kernel, dim3(nblk((long long)width * height)), dim3(NT), 0, ST, face_id, faces, (int)num_faces, pix_f, pix_q,
                       (int)num_verts, (int)width, (int)height, counts, pair_info);
    return check_launch("v3d_recon_mesh_aa_count");
}

extern "C" int v3d_recon_mesh_aa_emit(const int32_t* face_id, const int32_t* faces, int32_t num_faces, const float* pix_f, const int32_t* pix_q,
                                      int32_t num_verts, int32_t width, int32_t height, const float* alpha_raw, const float* dL_dalpha,
                                      const int32_t* offsets, int32_t num_records, uint64_t* keys, uint32_t* vals, float* payload,
                                      v3d_stream_t stream) {
    RECON_REQUIRE(face_id && faces && pix_f && pix_q && alpha_raw && dL_dalpha && offsets && keys && vals && payload,
                  "v3d_recon_mesh_aa_emit: null argument");
    AA_REQUIRE_MESH("v3d_recon_mesh_aa_emit", num_faces, num_verts);
    AA_REQUIRE_IMAGE("v3d_recon_mesh_aa_emit", width, height);
    const long long HW = (long long)width * height;
    RECON_REQUIRE(num_records > 0 && num_records % 2 == 0 && num_records <= 8 * HW,
                  "v3d_recon_mesh_aa_emit: num_records %d is not a positive multiple of 2 up to 8 x the pixel count", (int)num_records);
    hipLaunchKernelGGL(mesh_aa_emit_kernel, dim3(nblk(HW)), dim3(NT), 0, ST, face_id, faces, (int)num_faces, pix_f, pix_q, (int)num_verts, (int)width,
                       (int)height, alpha_raw, dL_dalpha, offsets, (int)num_records, (unsigned long long*)keys, vals, payload);
    return check_launch("v3d_recon_mesh_aa_emit");
}

extern "C" int v3d_recon_mesh_aa_reduce(const int32_t* ranges, const uint32_t* vals_sorted, const float* payload, int32_t num_records,
                                        int32_t num_verts, float* dL_dpix, v3d_stream_t stream) {
    RECON_REQUIRE(ranges && dL_dpix && ((vals_sorted && payload) || num_records == 0), "v3d_recon_mesh_aa_reduce: null argument");
    RECON_REQUIRE(num_records >= 0, "v3d_recon_mesh_aa_reduce: num_records must not be negative");
    RECON_REQUIRE(num_verts > 0, "v3d_recon_mesh_aa_reduce: num_verts must be positive");
    const long long blocks = ((long long)num_verts + NT / WAVE - 1) / (NT / WAVE);
    hipLaunchKernelGGL(mesh_aa_reduce_kernel, dim3((unsigned)blocks), dim3(NT), 0, ST, ranges, vals_sorted, payload, (int)num_records, (int)num_verts,
                       dL_dpix);
    return check_launch("v3d_recon_mesh_aa_reduce");
}

extern "C" int v3d_recon_mesh_project_bwd(const float* verts, int32_t num_verts, const v3d_gs_camera* cam, const int32_t* pix_q, const float* dL_dpix,
                                          float* dL_dverts, v3d_stream_t stream) {
    RECON_REQUIRE(verts && cam && pix_q && dL_dpix && dL_dverts, "v3d_recon_mesh_project_bwd: null argument");
    RECON_REQUIRE(num_verts > 0, "v3d_recon_mesh_project_bwd: num_verts must be positive");
    AA_REQUIRE_IMAGE("v3d_recon_mesh_project_bwd", cam->width, cam->height);
    hipLaunchKernelGGL(mesh_project_bwd_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, verts, (int)num_verts, *cam, pix_q, dL_dpix, dL_dverts);
    return check_launch("v3d_recon_mesh_project_bwd");
}

extern "C" int v3d_recon_mesh_smooth_grad(const float* offsets, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                          const int32_t* corners, float scale, float* grad, v3d_stream_t stream) {
    RECON_REQUIRE(offsets && faces && ranges && corners && grad, "v3d_recon_mesh_smooth_grad: null argument");
    RECON_REQUIRE(num_verts > 0 && num_faces > 0 && num_faces <= INT32_MAX / 3,
                  "v3d_recon_mesh_smooth_grad: num_verts %d and num_faces %d must be positive, 3 x num_faces at most INT32_MAX", (int)num_verts,
                  (int)num_faces);
    hipLaunchKernelGGL(mesh_smooth_grad_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, offsets, (int)num_verts, faces, (int)num_faces, ranges, corners,
                       scale, grad);
    return check_launch("v3d_recon_mesh_smooth_grad");
}
