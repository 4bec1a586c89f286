// Inside or outside: the generalized winding number on the tree of meshbvh.hip (include/v3d_recon.h "Mesh solid", libv3d_recon.so; host
// side: v3d_amd/recon/mesh_solid.py).  Jacobson, Kavan and Sorkine-Hornung, "Robust Inside-Outside Segmentation using Generalized Winding
// Numbers" (SIGGRAPH 2013) for the sum of solid angles, and the first order of Barill, Dickson, Schmidt, Levin and Jacobson, "Fast Winding
// Numbers for Soups and Clouds" (SIGGRAPH 2018) for the tree: a node far enough from the query stands for everything below it as one dipole.
// Both written from the papers.  moment_round fills a row of moments per node bottom-up (the fit's two `done` buffers, one more entry per
// leaf);  winding walks the tree per query;  sdf_grid runs the closest-point walk of bvh_walk.h and then the winding walk per voxel of a
// TSDF volume (geom.hip's layout) and writes the four arrays that v3d_recon_cells_flag and its successors read.
//
// No atomics.  The moments run between two `done` buffers, so no launch reads a row it writes.  A query's sum is taken in the order of the
// walk (left descended, right pushed), which is a function of the tree alone, and accumulated in double: on this chip an fp64 add costs
// little beside the atan2f or the divide that produced the term, and the result stops depending on the order to far below a float's ulp.
//
// The stacks live in LDS as in meshbvh.hip: stack[entry * 64 + lane], 16 KB to a block of one wave.  sdf_grid's wave is a 4 x 4 x 4 brick
// of voxels, so its 64 walks start within four voxels of each other and diverge late;  a row of 64 voxels would span a quarter of a
// 256-voxel volume.  The two walks of a voxel use the same column one after the other.
// Built without -ffast-math (v3d_amd/build.py): everything is held to an fp64 restatement (tests/mesh_solid_ref.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "bvh_walk.h"
#include "recon_host.h"
#include "v3d_recon.h"

namespace {

constexpr int MOM = 8;                             // floats to a row of THE MOMENTS: nx ny nz r2 cx cy cz area
constexpr double FOUR_PI = 12.566370614359172;

// ---------------------------------------------------------------------------------------------------------------------------------------
// Moments.  One thread per node; done_in, done_out [2F-1] (leaves included, unlike the fit's).
__device__ __forceinline__ float far_corner2(const float* lo, const float* hi, float cx, float cy, float cz) {
    if (!(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) return 0.f;     // the empty box
    const float ax = fmaxf((cx - lo[0]) * (cx - lo[0]), (hi[0] - cx) * (hi[0] - cx));
    const float ay = fmaxf((cy - lo[1]) * (cy - lo[1]), (hi[1] - cy) * (hi[1] - cy));
    const float az = fmaxf((cz - lo[2]) * (cz - lo[2]), (hi[2] - cz) * (hi[2] - cz));
    return (ax + ay) + az;
}

__global__ void __launch_bounds__(BT) bvh_moment_round_kernel(Tree tr, const int32_t* __restrict__ done_in, int32_t* __restrict__ done_out, float* mom,
                                                              int32_t* __restrict__ changed) {
    const long long i = (long long)blockIdx.x * BT + threadIdx.x;
    const int inner = tr.nf - 1, nodes = 2 * tr.nf - 1;
    if (i >= nodes) return;
    if (done_in[i]) {
        done_out[i] = 1;
        return;
    }
    const float* lo = tr.lo + 3 * i;
    const float* hi = tr.hi + 3 * i;
    float nx = 0.f, ny = 0.f, nz = 0.f, cx = 0.f, cy = 0.f, cz = 0.f, area = 0.f, r2 = 0.f;
    bool ready = true;
    if (i >= inner) {
        const uint32_t f = (uint32_t)tr.order[i - inner];
        if (f < (uint32_t)tr.nf) {
            const int i0 = tr.faces[3 * (long long)f], i1 = tr.faces[3 * (long long)f + 1], i2 = tr.faces[3 * (long long)f + 2];
            if (vert_ok(i0, tr.nv) && vert_ok(i1, tr.nv) && vert_ok(i2, tr.nv)) {
                const float* a = tr.verts + 3 * (long long)i0;
                const float* b = tr.verts + 3 * (long long)i1;
                const float* c = tr.verts + 3 * (long long)i2;
                const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
                const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
                if (!no_area(e1x, e1y, e1z, e2x, e2y, e2z)) {       // (a difference of equal products would be fused and leave a rounding error)
                    nx = 0.5f * (e1y * e2z - e1z * e2y), ny = 0.5f * (e1z * e2x - e1x * e2z), nz = 0.5f * (e1x * e2y - e1y * e2x);
                    area = sqrtf(dot3(nx, ny, nz, nx, ny, nz));
                }
                cx = ((a[0] + b[0]) + c[0]) / 3.f, cy = ((a[1] + b[1]) + c[1]) / 3.f, cz = ((a[2] + b[2]) + c[2]) / 3.f;
                r2 = far_corner2(lo, hi, cx, cy, cz);
            }
        }
    } else {
        const int a = tr.left[i], b = tr.right[i];
        ready = a >= 0 && a < nodes && b >= 0 && b < nodes && done_in[a] && done_in[b];
        if (ready) {
            const float* ma = mom + MOM * (long long)a;
            const float* mb = mom + MOM * (long long)b;
            nx = ma[0] + mb[0], ny = ma[1] + mb[1], nz = ma[2] + mb[2];
            area = ma[7] + mb[7];
            if (area > 0.f) {
                cx = (ma[7] * ma[4] + mb[7] * mb[4]) / area, cy = (ma[7] * ma[5] + mb[7] * mb[5]) / area, cz = (ma[7] * ma[6] + mb[7] * mb[6]) / area;
            } else if (lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2]) {
                cx = 0.5f * (lo[0] + hi[0]), cy = 0.5f * (lo[1] + hi[1]), cz = 0.5f * (lo[2] + hi[2]);
            }
            r2 = far_corner2(lo, hi, cx, cy, cz);
        }
    }
    if (ready) {
        float* m = mom + MOM * i;
        m[0] = nx, m[1] = ny, m[2] = nz, m[3] = r2, m[4] = cx, m[5] = cy, m[6] = cz, m[7] = area;
        *changed = 1;                              // (every writer stores the same value)
    }
    done_out[i] = ready ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// THE WINDING NUMBER of the header: the signed solid angle of one triangle seen from q, 0 for a face that is not one.
__device__ __forceinline__ float solid_angle(const Tree& tr, int face, float qx, float qy, float qz) {
    if (face < 0 || face >= tr.nf) return 0.f;
    const int i0 = tr.faces[3 * (long long)face], i1 = tr.faces[3 * (long long)face + 1], i2 = tr.faces[3 * (long long)face + 2];
    if (!(vert_ok(i0, tr.nv) && vert_ok(i1, tr.nv) && vert_ok(i2, tr.nv))) return 0.f;
    const float* v0 = tr.verts + 3 * (long long)i0;
    const float* v1 = tr.verts + 3 * (long long)i1;
    const float* v2 = tr.verts + 3 * (long long)i2;
    const float ax = v0[0] - qx, ay = v0[1] - qy, az = v0[2] - qz;
    const float bx = v1[0] - qx, by = v1[1] - qy, bz = v1[2] - qz;
    const float cx = v2[0] - qx, cy = v2[1] - qy, cz = v2[2] - qz;
    const float num = dot3(ax, ay, az, by * cz - bz * cy, bz * cx - bx * cz, bx * cy - by * cx);
    if (num == 0.f) return 0.f;                    // a query in the triangle's plane, on the triangle or beside it
    const float la = sqrtf(dot3(ax, ay, az, ax, ay, az)), lb = sqrtf(dot3(bx, by, bz, bx, by, bz)), lc = sqrtf(dot3(cx, cy, cz, cx, cy, cz));
    const float den = la * lb * lc + dot3(ax, ay, az, bx, by, bz) * lc + dot3(bx, by, bz, cx, cy, cz) * la + dot3(cx, cy, cz, ax, ay, az) * lb;
    return 2.f * atan2f(num, den);
}

// THE SUM.  Left is descended and right pushed: the order of the terms is the tree's.  Bounded as the other walks are.
__device__ float winding(const Tree& tr, const float* __restrict__ mom, float qx, float qy, float qz, float beta2, int* stack) {
    const int inner = tr.nf - 1, nodes = 2 * tr.nf - 1;
    double sum = 0.0;
    int sp = 0, node = 0;
    for (int step = 0; step < nodes; ++step) {
        bool pop = true;
        const float* m = mom + MOM * (long long)node;
        if (m[7] == 0.f) {
            // nothing below has area: no term, no descent
        } else {
            const float dx = m[4] - qx, dy = m[5] - qy, dz = m[6] - qz;
            const float d2 = dot3(dx, dy, dz, dx, dy, dz);
            if (beta2 > 0.f && d2 > beta2 * m[3]) {
                sum += (double)(dot3(m[0], m[1], m[2], dx, dy, dz) / (d2 * sqrtf(d2)));
            } else if (node >= inner) {
                const uint32_t f = (uint32_t)tr.order[node - inner];
                sum += (double)solid_angle(tr, f < (uint32_t)tr.nf ? (int)f : -1, qx, qy, qz);
            } else {
                const int a = tr.left[node], b = tr.right[node];
                const bool oa = a >= 0 && a < nodes, ob = b >= 0 && b < nodes;
                if (oa && ob) {
                    if (sp < STACK) stack[BT * sp++] = b;
                    node = a;
                    pop = false;
                } else if (oa || ob) {
                    node = oa ? a : b;
                    pop = false;
                }
            }
        }
        if (pop) {
            if (sp == 0) break;
            node = stack[BT * --sp];
        }
    }
    return (float)(sum / FOUR_PI);
}

__global__ void __launch_bounds__(BT) bvh_winding_kernel(Tree tr, const float* __restrict__ mom, const float* __restrict__ points, int n, float beta2,
                                                         float* __restrict__ w) {
    __shared__ int stack[STACK * BT];
    const long long i = (long long)blockIdx.x * BT + threadIdx.x;
    if (i >= n) return;
    const float px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
    w[i] = isfinite(px) && isfinite(py) && isfinite(pz) ? winding(tr, mom, px, py, pz, beta2, stack + threadIdx.x) : NAN;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The volume.  The centre is geom.hip's voxel_centre written as the fused multiply-add the compiler makes of it anyway: one rounding of the
// exact value, which the host can form in double (the product of a float and a half-integer below 2^10 is exact there, and so is the sum).
__device__ __forceinline__ float brick_centre(int i, float voxel, float bound) { return fmaf((float)i + 0.5f, voxel, -bound); }

__global__ void __launch_bounds__(BT) sdf_grid_kernel(Tree tr, const float* __restrict__ mom, const float* __restrict__ colors, int N, float bound, float voxel,
                                                      float trunc, float beta2, float* __restrict__ tsdf_sum, float* __restrict__ weight,
                                                      float* __restrict__ rgb_sum, float* __restrict__ rgb_weight) {
    __shared__ int stack[STACK * BT];
    const int lane = threadIdx.x;
    const int ix = 4 * (int)blockIdx.x + (lane & 3), iy = 4 * (int)blockIdx.y + ((lane >> 2) & 3), iz = 4 * (int)blockIdx.z + (lane >> 4);
    if (ix >= N || iy >= N || iz >= N) return;
    const float px = brick_centre(ix, voxel, bound), py = brick_centre(iy, voxel, bound), pz = brick_centre(iz, voxel, bound);
    const Near h = closest_point(tr, px, py, pz, trunc * trunc, stack + lane);
    const float w = winding(tr, mom, px, py, pz, beta2, stack + lane);
    const float s = w >= 0.5f ? -1.f : 1.f;        // (a NaN w is outside)
    const bool found = h.face >= 0;
    float r = 0.f, g = 0.f, b = 0.f;
    if (found && colors) {                         // (closest_point returns only faces whose indices are vertices)
        const float w0 = 1.f - h.u - h.v;
        const float *c0 = colors + 3 * (long long)tr.faces[3 * (long long)h.face], *c1 = colors + 3 * (long long)tr.faces[3 * (long long)h.face + 1],
                    *c2 = colors + 3 * (long long)tr.faces[3 * (long long)h.face + 2];
        r = w0 * c0[0] + h.u * c1[0] + h.v * c2[0];
        g = w0 * c0[1] + h.u * c1[1] + h.v * c2[1];
        b = w0 * c0[2] + h.u * c1[2] + h.v * c2[2];
    }
    const long long n3 = (long long)N * N * N, o = ((long long)iz * N + iy) * N + ix;
    tsdf_sum[o] = found ? s * fminf(sqrtf(h.d2) / trunc, 1.f) : s;
    weight[o] = 1.f;
    rgb_sum[o] = r;
    rgb_sum[n3 + o] = g;
    rgb_sum[2 * n3 + o] = b;
    rgb_weight[o] = found && colors ? 1.f : 0.f;
}

bool beta_ok(float beta) { return beta >= 0.f && isfinite(beta); }

}  // namespace

extern "C" int v3d_recon_bvh_moment_round(const int32_t* left, const int32_t* right, const uint32_t* order, const float* lo, const float* hi,
                                          const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* done_in,
                                          int32_t* done_out, float* mom, int32_t* changed, v3d_stream_t stream) {
    RECON_REQUIRE(done_in && done_out && mom && changed, "v3d_recon_bvh_moment_round: null argument");
    BVH_REQUIRE_TREE("v3d_recon_bvh_moment_round", left, right, order, lo, hi, verts, num_verts, faces, num_faces);
    RECON_REQUIRE(done_in != done_out, "v3d_recon_bvh_moment_round: done_in and done_out must be two buffers");
    const Tree tr{left, right, (const int32_t*)order, lo, hi, verts, faces, (int)num_verts, (int)num_faces};
    hipLaunchKernelGGL(bvh_moment_round_kernel, dim3(nblk_bt(2LL * num_faces - 1)), dim3(BT), 0, ST, tr, done_in, done_out, mom, changed);
    return check_launch("v3d_recon_bvh_moment_round");
}

extern "C" int v3d_recon_bvh_winding(const float* points, int32_t num_points, float beta, const int32_t* left, const int32_t* right, const uint32_t* order,
                                     const float* lo, const float* hi, const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces,
                                     const float* mom, float* w, v3d_stream_t stream) {
    RECON_REQUIRE(points && mom && w, "v3d_recon_bvh_winding: null argument");
    BVH_REQUIRE_TREE("v3d_recon_bvh_winding", left, right, order, lo, hi, verts, num_verts, faces, num_faces);
    RECON_REQUIRE(num_points > 0, "v3d_recon_bvh_winding: num_points must be positive");
    RECON_REQUIRE(beta_ok(beta), "v3d_recon_bvh_winding: beta %g must be finite and not negative", (double)beta);
    const Tree tr{left, right, (const int32_t*)order, lo, hi, verts, faces, (int)num_verts, (int)num_faces};
    hipLaunchKernelGGL(bvh_winding_kernel, dim3(nblk_bt(num_points)), dim3(BT), 0, ST, tr, mom, points, (int)num_points, beta * beta, w);
    return check_launch("v3d_recon_bvh_winding");
}

extern "C" int v3d_recon_sdf_grid(const int32_t* left, const int32_t* right, const uint32_t* order, const float* lo, const float* hi, const float* verts,
                                  int32_t num_verts, const int32_t* faces, int32_t num_faces, const float* mom, const float* colors, int32_t N, float bound,
                                  float trunc, float beta, float* tsdf_sum, float* weight, float* rgb_sum, float* rgb_weight, v3d_stream_t stream) {
    RECON_REQUIRE(mom && tsdf_sum && weight && rgb_sum && rgb_weight, "v3d_recon_sdf_grid: null argument");
    BVH_REQUIRE_TREE("v3d_recon_sdf_grid", left, right, order, lo, hi, verts, num_verts, faces, num_faces);
    RECON_REQUIRE(N >= 2 && N <= V3D_RECON_MAX_N, "v3d_recon_sdf_grid: resolution %d outside 2 .. %d (voxel indices are int32)", (int)N, V3D_RECON_MAX_N);
    RECON_REQUIRE(bound > 0.f && isfinite(bound), "v3d_recon_sdf_grid: bound %g must be finite and positive", (double)bound);
    RECON_REQUIRE(trunc > 0.f && isfinite(trunc), "v3d_recon_sdf_grid: trunc %g must be finite and positive", (double)trunc);
    RECON_REQUIRE(beta_ok(beta), "v3d_recon_sdf_grid: beta %g must be finite and not negative", (double)beta);
    const Tree tr{left, right, (const int32_t*)order, lo, hi, verts, faces, (int)num_verts, (int)num_faces};
    const unsigned bricks = (unsigned)((N + 3) / 4);
    hipLaunchKernelGGL(sdf_grid_kernel, dim3(bricks, bricks, bricks), dim3(BT), 0, ST, tr, mom, colors, (int)N, bound, 2.f * bound / (float)N, trunc,
                       beta * beta, tsdf_sum, weight, rgb_sum, rgb_weight);
    return check_launch("v3d_recon_sdf_grid");
}
