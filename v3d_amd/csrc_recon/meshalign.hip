// The hot step of mesh registration on the tree of meshbvh.hip (include/v3d_recon.h "Mesh alignment", libv3d_recon.so; host side:
// v3d_amd/recon/mesh_align.py): align_correspond moves every sample by a similarity, finds its closest point on the tree's mesh with the
// walk of bvh_walk.h (the very closest_point behind v3d_recon_bvh_closest_point) and reduces the 20 weighted moments of the pairs to one
// row per block;  align_reduce adds the rows.  The host solves the next similarity from the 20 sums (Umeyama), so an iteration reads back
// 160 bytes.
//
// No atomics.  A row is the sum over one wave by the xor butterfly (v += shfl_xor(v, o), o = 32 .. 1): both partners of a step add the same
// two doubles, so every lane ends with the same bits whatever the order, and the rows are added by one block in a fixed order.
//
// The stack lives in LDS as in meshquery.hip: 16 KB to a block of one wave, 10 waves to a CU, stack[entry * 64 + lane] with lane l on bank
// l mod 32 whatever its depth.  A block is one wave, so the reduction needs no LDS of its own and no barrier.  A 64-bit shuffle is two
// 32-bit ds_bpermute: 20 columns x 6 steps x 2 = 240 per wave, once, after a walk that visits some hundreds of nodes per lane;  the 20
// doubles (40 VGPRs) live only after the walk has returned, so they do not press on the walk's registers.  No lane leaves before the
// butterfly: a lane past N carries zeros.
// Built without -ffast-math (v3d_amd/build.py);  the terms are formed with contraction off so that the host can restate every one of
// them bit for bit (tests/mesh_align_ref.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "bvh_walk.h"
#include "recon_host.h"
#include "v3d_recon.h"

namespace {

constexpr int COLS = V3D_RECON_ALIGN_COLUMNS;

struct Xf {
    float m[12];
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = BT / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, BT);
    return v;
}

// The 20 terms of a sample that counts, every operation rounded on its own.
__device__ __forceinline__ void pair_terms(float wf, const float* p, const float* q, float distf, double* t) {
#pragma clang fp contract(off)
    const double w = (double)wf, d = (double)distf;
    const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
    t[0] = w;
    t[1] = w * px, t[2] = w * py, t[3] = w * pz;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double wq = w * (double)q[i];
        t[4 + i] = wq;
        t[7 + 3 * i] = wq * px, t[8 + 3 * i] = wq * py, t[9 + 3 * i] = wq * pz;
    }
    t[16] = w * ((px * px + py * py) + pz * pz);
    t[17] = w * (d * d);
    t[18] = 1.0;
}

__global__ void __launch_bounds__(BT) align_correspond_kernel(Tree tr, const float* __restrict__ points, const float* __restrict__ weights, int n, Xf xf,
                                                              float max_d2, float* __restrict__ moved, float* __restrict__ closest,
                                                              float* __restrict__ dist, int32_t* __restrict__ face, float* __restrict__ uv,
                                                              double* __restrict__ partials) {
    __shared__ int stack[STACK * BT];
    const long long i = (long long)blockIdx.x * BT + threadIdx.x;
    double t[COLS];
#pragma unroll
    for (int c = 0; c < COLS; ++c) t[c] = 0.0;
    if (i < n) {
        const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2], w = weights[i];
        float p[3], q[3] = {NAN, NAN, NAN};
#pragma unroll
        for (int r = 0; r < 3; ++r) p[r] = ((xf.m[4 * r] * x + xf.m[4 * r + 1] * y) + xf.m[4 * r + 2] * z) + xf.m[4 * r + 3];
        const bool finite = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
        Near h{INFINITY, 0.f, 0.f, -1};
        if (finite) h = closest_point(tr, p[0], p[1], p[2], max_d2, stack + threadIdx.x);
        const bool found = h.face >= 0;
        const float d = found ? sqrtf(h.d2) : INFINITY;
        if (found) {                                   // (a face that closest_point returns has passed near_triangle's index checks)
            const float* a = tr.verts + 3 * (long long)tr.faces[3 * (long long)h.face];
            const float* b = tr.verts + 3 * (long long)tr.faces[3 * (long long)h.face + 1];
            const float* c = tr.verts + 3 * (long long)tr.faces[3 * (long long)h.face + 2];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                q[r] = a[r] + h.u * (b[r] - a[r]) + h.v * (c[r] - a[r]);
                if (h.u == 1.f) q[r] = b[r];
                if (h.v == 1.f) q[r] = c[r];
            }
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) moved[3 * i + r] = p[r], closest[3 * i + r] = q[r];
        dist[i] = d;
        face[i] = found ? h.face : -1;
        uv[2 * i] = found ? h.u : 0.f;
        uv[2 * i + 1] = found ? h.v : 0.f;
        const bool valid = finite && isfinite(w) && w >= 0.f;
        if (valid && found) pair_terms(w, p, q, d, t);
        if (valid) t[19] = (double)w;
    }
#pragma unroll
    for (int c = 0; c < COLS; ++c) t[c] = wave_sum_f64(t[c]);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < COLS; ++c) partials[(long long)blockIdx.x * COLS + c] = t[c];
    }
}

__global__ void __launch_bounds__(BT) align_reduce_kernel(const double* __restrict__ partials, int rows, double* __restrict__ sums) {
    double t[COLS];
#pragma unroll
    for (int c = 0; c < COLS; ++c) t[c] = 0.0;
    for (long long r = threadIdx.x; r < rows; r += BT) {
#pragma unroll
        for (int c = 0; c < COLS; ++c) t[c] += partials[r * COLS + c];
    }
#pragma unroll
    for (int c = 0; c < COLS; ++c) t[c] = wave_sum_f64(t[c]);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < COLS; ++c) sums[c] = t[c];
    }
}

}  // namespace

extern "C" int v3d_recon_align_correspond(const float* points, const float* weights, int32_t num_points, const float* xf, float max_dist,
                                          const int32_t* left, const int32_t* right, const uint32_t* order, const float* lo, const float* hi,
                                          const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, float* moved, float* closest,
                                          float* dist, int32_t* face, float* uv, double* partials, v3d_stream_t stream) {
    RECON_REQUIRE(points && weights && xf && moved && closest && dist && face && uv && partials, "v3d_recon_align_correspond: null argument");
    BVH_REQUIRE_TREE("v3d_recon_align_correspond", left, right, order, lo, hi, verts, num_verts, faces, num_faces);
    RECON_REQUIRE(num_points > 0, "v3d_recon_align_correspond: num_points must be positive");
    RECON_REQUIRE(max_dist >= 0.f, "v3d_recon_align_correspond: max_dist %g must not be negative or NaN", (double)max_dist);
    Xf m;
    for (int k = 0; k < 12; ++k) m.m[k] = xf[k];
    const Tree tr{left, right, (const int32_t*)order, lo, hi, verts, faces, (int)num_verts, (int)num_faces};
    hipLaunchKernelGGL(align_correspond_kernel, dim3(nblk_bt(num_points)), dim3(BT), 0, ST, tr, points, weights, (int)num_points, m, max_dist * max_dist,
                       moved, closest, dist, face, uv, partials);
    return check_launch("v3d_recon_align_correspond");
}

extern "C" int v3d_recon_align_reduce(const double* partials, int32_t num_rows, double* sums, v3d_stream_t stream) {
    RECON_REQUIRE(partials && sums, "v3d_recon_align_reduce: null argument");
    RECON_REQUIRE(num_rows > 0, "v3d_recon_align_reduce: num_rows must be positive");
    hipLaunchKernelGGL(align_reduce_kernel, dim3(1), dim3(BT), 0, ST, partials, (int)num_rows, sums);
    return check_launch("v3d_recon_align_reduce");
}
