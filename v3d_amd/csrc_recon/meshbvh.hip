// Ray queries of one mesh against another (include/v3d_recon.h "Mesh BVH and normal bake", libv3d_recon.so; host side:
// v3d_amd/recon/mesh_bake.py).  A linear bounding-volume hierarchy after Karras, "Maximizing Parallelism in the Construction of BVHs, Octrees,
// and k-d Trees" (HPG 2012), written from the paper: face_keys (a box and a 30-bit Morton code per face) -> v3d_gs_radix_sort_pairs (stable)
// -> build_nodes (one thread per internal node finds its range by the common-prefix function and splits it) -> fit_round until nothing
// changes (an internal node takes the union of its children's boxes once both are done).  closest_hit walks the tree with a stack per ray;
// tex_bake_normals casts two rays per texel of the low mesh's atlas (meshtex.hip's ownership rule) against the high mesh.
//
// No atomics: the fit runs between two `done` buffers, so no launch reads what it writes, and min / max are exact, so the boxes do not
// depend on the order of anything.  The traversal's result is the smallest t over the triangle tests and, on equal t, the smaller face: a
// function of the set of triangles tested, not of their order, and the box test only ever leaves out triangles the ray cannot reach.
//
// The stack lives in LDS, stack[entry][lane]: 64 entries x 64 lanes x 4 bytes = 16 KB to a block of one wave.  A private array indexed at
// run time would go to scratch memory.  The LDS per wave is the same at any block size, so occupancy is too (10 waves to a CU's 160 KB);
// one wave to a block lets a block retire as soon as its own rays are done instead of waiting for the slowest of four waves.
// Built without -ffast-math (v3d_amd/build.py): everything is held to an fp64 restatement (tests/mesh_bake_ref.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "bvh_walk.h"
#include "recon_host.h"
#include "v3d_recon.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------------------------
// Keys.  Bits of x spread to every third place: 10 bits in, 28 bits out.
__device__ __forceinline__ uint32_t spread3(uint32_t x) {
    x &= 0x3ffu;
    x = (x | (x << 16)) & 0x030000ffu;
    x = (x | (x << 8)) & 0x0300f00fu;
    x = (x | (x << 4)) & 0x030c30c3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// 0 .. 1023; 0 for a NaN centre (an empty box) and for a mesh without extent on this axis (scale 0)
__device__ __forceinline__ uint32_t quantise(float c, float lo, float scale) {
    const float x = (c - lo) * scale;
    return x > 0.f ? (x < 1023.f ? (uint32_t)x : 1023u) : 0u;
}

__global__ void __launch_bounds__(NT) bvh_face_keys_kernel(const float* __restrict__ verts, int nv, const int32_t* __restrict__ faces, int nf, float lx, float ly,
                                                           float lz, float sx, float sy, float sz, unsigned long long* __restrict__ keys,
                                                           uint32_t* __restrict__ vals, float* __restrict__ face_lo, float* __restrict__ face_hi) {
    const long long f = (long long)blockIdx.x * NT + threadIdx.x;
    if (f >= nf) return;
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};          // empty: never entered, never hit
    if (vert_ok(i0, nv) && vert_ok(i1, nv) && vert_ok(i2, nv)) {
        for (int k = 0; k < 3; ++k) {
            const float a = verts[3 * (long long)i0 + k], b = verts[3 * (long long)i1 + k], c = verts[3 * (long long)i2 + k];
            lo[k] = fminf(a, fminf(b, c));
            hi[k] = fmaxf(a, fmaxf(b, c));
        }
    }
    const uint32_t qx = quantise(0.5f * (lo[0] + hi[0]), lx, sx), qy = quantise(0.5f * (lo[1] + hi[1]), ly, sy), qz = quantise(0.5f * (lo[2] + hi[2]), lz, sz);
    keys[f] = (unsigned long long)((spread3(qx) << 2) | (spread3(qy) << 1) | spread3(qz));
    vals[f] = (uint32_t)f;
    for (int k = 0; k < 3; ++k) {
        face_lo[3 * f + k] = lo[k];
        face_hi[3 * f + k] = hi[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Nodes.  delta(i, j): the length of the common prefix of the sorted keys i and j, -1 outside 0 .. F-1; equal codes are told apart by the
// sorted position, 32 + clz(i ^ j), so every pair of distinct positions has a finite delta and the ranges nest as in the paper.
__device__ __forceinline__ int delta(const unsigned long long* __restrict__ keys, long long nf, long long i, long long j) {
    if (j < 0 || j >= nf) return -1;
    const uint32_t a = (uint32_t)keys[i], b = (uint32_t)keys[j];
    return a != b ? __clz((int)(a ^ b)) : 32 + __clz((int)((uint32_t)i ^ (uint32_t)j));
}

// Thread i < F - 1 builds internal node i; every thread i < F places leaf i (node F - 1 + i): its face's box, in sorted order.
__global__ void __launch_bounds__(NT) bvh_build_nodes_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ order,
                                                             const float* __restrict__ face_lo, const float* __restrict__ face_hi, int nf,
                                                             int32_t* __restrict__ left, int32_t* __restrict__ right, int32_t* __restrict__ parent,
                                                             float* __restrict__ lo, float* __restrict__ hi) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= nf) return;
    const long long leaf = (long long)nf - 1 + i;
    const uint32_t f = order[i];
    for (int k = 0; k < 3; ++k) {
        const bool ok = f < (uint32_t)nf;
        lo[3 * leaf + k] = ok ? face_lo[3 * (long long)f + k] : INFINITY;
        hi[3 * leaf + k] = ok ? face_hi[3 * (long long)f + k] : -INFINITY;
    }
    if (i == 0) parent[0] = -1;                    // the root: node 0, which is the lone leaf when F = 1
    if (i >= nf - 1) return;
    const int d = delta(keys, nf, i, i + 1) - delta(keys, nf, i, i - 1) >= 0 ? 1 : -1;
    const int dmin = delta(keys, nf, i, i - d);
    long long lmax = 2;
    while (delta(keys, nf, i, i + lmax * d) > dmin) lmax *= 2;
    long long l = 0;
    for (long long t = lmax / 2; t >= 1; t /= 2)
        if (delta(keys, nf, i, i + (l + t) * d) > dmin) l += t;
    const long long j = i + l * d;
    const int dnode = delta(keys, nf, i, j);
    long long s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (delta(keys, nf, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    long long gamma = i + s * d + (d < 0 ? -1 : 0);
    gamma = gamma < 0 ? 0 : (gamma > nf - 2 ? nf - 2 : gamma);                 // (inside already, on sorted keys)
    const long long first = i < j ? i : j, last = i < j ? j : i;
    const long long a = first == gamma ? nf - 1 + gamma : gamma, b = last == gamma + 1 ? nf - 1 + gamma + 1 : gamma + 1;
    left[i] = (int32_t)a;
    right[i] = (int32_t)b;
    parent[a] = (int32_t)i;
    parent[b] = (int32_t)i;
}

// One thread per internal node.  A leaf is always done.
__global__ void __launch_bounds__(NT) bvh_fit_round_kernel(const int32_t* __restrict__ left, const int32_t* __restrict__ right, int nf,
                                                           const int32_t* __restrict__ done_in, int32_t* __restrict__ done_out, float* lo, float* hi,
                                                           int32_t* __restrict__ changed) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= nf - 1) return;
    if (done_in[i]) {
        done_out[i] = 1;
        return;
    }
    const int a = left[i], b = right[i], n = 2 * nf - 1;
    const bool ready = a >= 0 && a < n && b >= 0 && b < n && (a >= nf - 1 || done_in[a]) && (b >= nf - 1 || done_in[b]);
    if (ready) {
        for (int k = 0; k < 3; ++k) {
            lo[3 * i + k] = fminf(lo[3 * (long long)a + k], lo[3 * (long long)b + k]);
            hi[3 * i + k] = fmaxf(hi[3 * (long long)a + k], hi[3 * (long long)b + k]);
        }
        *changed = 1;                              // (every writer stores the same value)
    }
    done_out[i] = ready ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Closest hit.  The tree's arguments, the tests and the walk are in bvh_walk.h, which meshquery.hip shares.
__global__ void __launch_bounds__(BT) bvh_closest_hit_kernel(Tree tr, const float* __restrict__ rays_o, const float* __restrict__ rays_d, float tmin,
                                                             float tmax, int n, int cull, float* __restrict__ t, int32_t* __restrict__ face,
                                                             float* __restrict__ uv) {
    __shared__ int stack[STACK * BT];
    const long long i = (long long)blockIdx.x * BT + threadIdx.x;
    if (i >= n) return;
    const Ray r = make_ray(rays_o[3 * i], rays_o[3 * i + 1], rays_o[3 * i + 2], rays_d[3 * i], rays_d[3 * i + 1], rays_d[3 * i + 2]);
    const Hit h = closest_hit(tr, r, tmin, tmax, cull, false, stack + threadIdx.x);
    t[i] = h.t;
    face[i] = h.face;
    uv[2 * i] = h.u;
    uv[2 * i + 1] = h.v;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The bake.  The atlas arithmetic is meshtex.hip's tex_bake_kernel, statement for statement.
__global__ void __launch_bounds__(BT) tex_bake_normals_kernel(int R, int S, int g, int F, const float* __restrict__ lverts, int lnv,
                                                              const int32_t* __restrict__ lfaces, const float* __restrict__ lnormals, float max_dist, Tree tr,
                                                              const float* __restrict__ hnormals, int32_t* __restrict__ owner,
                                                              float* __restrict__ normal_map, float* __restrict__ dist, int32_t* __restrict__ hit_face) {
    __shared__ int stack[STACK * BT];
    const long long t = (long long)blockIdx.x * BT + threadIdx.x;
    if (t >= (long long)R * R) return;
    const int x = (int)(t % R), y = (int)(t / R);
    int f = -1, hf = -1;
    float n0 = 0.f, n1 = 0.f, n2 = 1.f, sd = NAN;
    if (x < g * S && y < g * S) {
        const int cx = x / S, cy = y / S;
        int i = x - cx * S, j = y - cy * S;
        const int half = i + j <= S - 2 ? 0 : 1;
        const long long fl = 2LL * ((long long)cy * g + cx) + half;
        if (fl < F) {
            f = (int)fl;
            if (half) i = S - 1 - i, j = S - 1 - j;
            const int v0 = lfaces[3 * fl], v1 = lfaces[3 * fl + 1], v2 = lfaces[3 * fl + 2];
            if (vert_ok(v0, lnv) && vert_ok(v1, lnv) && vert_ok(v2, lnv)) {
                const float L = (float)(S - 3);
                const float b1 = fminf(fmaxf((float)i / L, 0.f), 1.f);
                const float b2 = fminf(fmaxf((float)j / L, 0.f), 1.f - b1);
                const float b0 = 1.f - b1 - b2;
                const float *p0 = lverts + 3 * (long long)v0, *p1 = lverts + 3 * (long long)v1, *p2 = lverts + 3 * (long long)v2;
                const float *m0 = lnormals + 3 * (long long)v0, *m1 = lnormals + 3 * (long long)v1, *m2 = lnormals + 3 * (long long)v2;
                const float px = b0 * p0[0] + b1 * p1[0] + b2 * p2[0], py = b0 * p0[1] + b1 * p1[1] + b2 * p2[1], pz = b0 * p0[2] + b1 * p1[2] + b2 * p2[2];
                n0 = b0 * m0[0] + b1 * m1[0] + b2 * m2[0];
                n1 = b0 * m0[1] + b1 * m1[1] + b2 * m2[1];
                n2 = b0 * m0[2] + b1 * m1[2] + b2 * m2[2];
                unit(n0, n1, n2);
                // outwards, then inwards: both accept only triangles whose geometric normal agrees with n
                const Hit hp = closest_hit(tr, make_ray(px, py, pz, n0, n1, n2), 0.f, max_dist, 2, false, stack + threadIdx.x);
                const Hit hm = closest_hit(tr, make_ray(px, py, pz, -n0, -n1, -n2), 0.f, max_dist, 1, true, stack + threadIdx.x);
                const bool plus = hp.face >= 0 && (hm.face < 0 || hp.t <= hm.t);
                const Hit h = plus ? hp : hm;
                if (h.face >= 0) {                 // (closest_hit returns only faces whose indices are vertices)
                    hf = h.face;
                    sd = plus ? h.t : -h.t;
                    const float w0 = 1.f - h.u - h.v;
                    const float *q0 = hnormals + 3 * (long long)tr.faces[3 * (long long)hf], *q1 = hnormals + 3 * (long long)tr.faces[3 * (long long)hf + 1],
                                *q2 = hnormals + 3 * (long long)tr.faces[3 * (long long)hf + 2];
                    n0 = w0 * q0[0] + h.u * q1[0] + h.v * q2[0];
                    n1 = w0 * q0[1] + h.u * q1[1] + h.v * q2[1];
                    n2 = w0 * q0[2] + h.u * q1[2] + h.v * q2[2];
                    unit(n0, n1, n2);
                }
            }
        }
    }
    owner[t] = f;
    hit_face[t] = hf;
    dist[t] = sd;
    normal_map[3 * t] = n0;
    normal_map[3 * t + 1] = n1;
    normal_map[3 * t + 2] = n2;
}

}  // namespace

extern "C" int v3d_recon_bvh_face_keys(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, float lo_x, float lo_y, float lo_z,
                                       float hi_x, float hi_y, float hi_z, uint64_t* keys, uint32_t* vals, float* face_lo, float* face_hi,
                                       v3d_stream_t stream) {
    RECON_REQUIRE(verts && faces && keys && vals && face_lo && face_hi, "v3d_recon_bvh_face_keys: null argument");
    RECON_REQUIRE(num_verts > 0, "v3d_recon_bvh_face_keys: num_verts must be positive");
    BVH_REQUIRE_FACES("v3d_recon_bvh_face_keys", num_faces);
    RECON_REQUIRE(hi_x >= lo_x && hi_y >= lo_y && hi_z >= lo_z && isfinite(hi_x - lo_x) && isfinite(hi_y - lo_y) && isfinite(hi_z - lo_z),
                  "v3d_recon_bvh_face_keys: the bounding box is not finite with lo <= hi");
    const float sx = hi_x > lo_x ? 1024.f / (hi_x - lo_x) : 0.f, sy = hi_y > lo_y ? 1024.f / (hi_y - lo_y) : 0.f,
                sz = hi_z > lo_z ? 1024.f / (hi_z - lo_z) : 0.f;
    hipLaunchKernelGGL(bvh_face_keys_kernel, dim3(nblk(num_faces)), dim3(NT), 0, ST, verts, (int)num_verts, faces, (int)num_faces, lo_x, lo_y, lo_z, sx, sy,
                       sz, (unsigned long long*)keys, vals, face_lo, face_hi);
    return check_launch("v3d_recon_bvh_face_keys");
}

extern "C" int v3d_recon_bvh_build_nodes(const uint64_t* keys_sorted, const uint32_t* order, const float* face_lo, const float* face_hi, int32_t num_faces,
                                         int32_t* left, int32_t* right, int32_t* parent, float* lo, float* hi, v3d_stream_t stream) {
    RECON_REQUIRE(keys_sorted && order && face_lo && face_hi && left && right && parent && lo && hi, "v3d_recon_bvh_build_nodes: null argument");
    BVH_REQUIRE_FACES("v3d_recon_bvh_build_nodes", num_faces);
    hipLaunchKernelGGL(bvh_build_nodes_kernel, dim3(nblk(num_faces)), dim3(NT), 0, ST, (const unsigned long long*)keys_sorted, order, face_lo, face_hi,
                       (int)num_faces, left, right, parent, lo, hi);
    return check_launch("v3d_recon_bvh_build_nodes");
}

extern "C" int v3d_recon_bvh_fit_round(const int32_t* left, const int32_t* right, int32_t num_faces, const int32_t* done_in, int32_t* done_out, float* lo,
                                       float* hi, int32_t* changed, v3d_stream_t stream) {
    RECON_REQUIRE(left && right && done_in && done_out && lo && hi && changed, "v3d_recon_bvh_fit_round: null argument");
    RECON_REQUIRE(done_in != done_out, "v3d_recon_bvh_fit_round: done_in and done_out must be two buffers");
    RECON_REQUIRE(num_faces >= 2 && num_faces <= BVH_MAX_FACES, "v3d_recon_bvh_fit_round: num_faces %d outside 2 .. %d (one face has no internal node)",
                  (int)num_faces, BVH_MAX_FACES);
    hipLaunchKernelGGL(bvh_fit_round_kernel, dim3(nblk(num_faces - 1)), dim3(NT), 0, ST, left, right, (int)num_faces, done_in, done_out, lo, hi, changed);
    return check_launch("v3d_recon_bvh_fit_round");
}

extern "C" int v3d_recon_bvh_closest_hit(const float* rays_o, const float* rays_d, float tmin, float tmax, int32_t num_rays, int32_t cull,
                                         const int32_t* left, const int32_t* right, const uint32_t* order, const float* lo, const float* hi,
                                         const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, float* t, int32_t* face, float* uv,
                                         v3d_stream_t stream) {
    RECON_REQUIRE(rays_o && rays_d && t && face && uv, "v3d_recon_bvh_closest_hit: null argument");
    BVH_REQUIRE_TREE("v3d_recon_bvh_closest_hit", left, right, order, lo, hi, verts, num_verts, faces, num_faces);
    RECON_REQUIRE(num_rays > 0, "v3d_recon_bvh_closest_hit: num_rays must be positive");
    RECON_REQUIRE(cull >= 0 && cull <= 2, "v3d_recon_bvh_closest_hit: cull %d outside 0 .. 2", (int)cull);
    RECON_REQUIRE(!(tmin != tmin) && !(tmax != tmax), "v3d_recon_bvh_closest_hit: tmin or tmax is NaN");
    const Tree tr{left, right, (const int32_t*)order, lo, hi, verts, faces, (int)num_verts, (int)num_faces};
    hipLaunchKernelGGL(bvh_closest_hit_kernel, dim3(nblk_bt(num_rays)), dim3(BT), 0, ST, tr, rays_o, rays_d, tmin, tmax, (int)num_rays, (int)cull, t, face,
                       uv);
    return check_launch("v3d_recon_bvh_closest_hit");
}

extern "C" int v3d_recon_tex_bake_normals(const float* low_verts, int32_t low_num_verts, const int32_t* low_faces, int32_t low_num_faces,
                                          const float* low_normals, int32_t tex_size, float max_dist, const int32_t* left, const int32_t* right,
                                          const uint32_t* order, const float* lo, const float* hi, const float* verts, int32_t num_verts,
                                          const int32_t* faces, int32_t num_faces, const float* normals, int32_t* owner, float* normal_map, float* dist,
                                          int32_t* hit_face, v3d_stream_t stream) {
    RECON_REQUIRE(low_verts && low_faces && low_normals && normals && owner && normal_map && dist && hit_face, "v3d_recon_tex_bake_normals: null argument");
    BVH_REQUIRE_TREE("v3d_recon_tex_bake_normals", left, right, order, lo, hi, verts, num_verts, faces, num_faces);
    RECON_REQUIRE(low_num_verts > 0, "v3d_recon_tex_bake_normals: low_num_verts must be positive");
    RECON_REQUIRE(low_num_faces > 0, "v3d_recon_tex_bake_normals: low_num_faces must be positive");
    RECON_REQUIRE(tex_size >= 1 && tex_size <= V3D_RECON_TEX_MAX_SIZE, "v3d_recon_tex_bake_normals: tex_size %d outside 1 .. %d", (int)tex_size,
                  V3D_RECON_TEX_MAX_SIZE);
    int S, g;
    RECON_REQUIRE(atlas_cells(low_num_faces, tex_size, &S, &g), "v3d_recon_tex_bake_normals: texture too small for %d faces: %d x %d leaves cells of %d texels, below %d",
                  (int)low_num_faces, (int)tex_size, (int)tex_size, S, V3D_RECON_TEX_MIN_CELL);
    RECON_REQUIRE(max_dist >= 0.f && isfinite(max_dist), "v3d_recon_tex_bake_normals: max_dist must be finite and not negative");
    const Tree tr{left, right, (const int32_t*)order, lo, hi, verts, faces, (int)num_verts, (int)num_faces};
    hipLaunchKernelGGL(tex_bake_normals_kernel, dim3(nblk_bt((long long)tex_size * tex_size)), dim3(BT), 0, ST, (int)tex_size, S, g, (int)low_num_faces,
                       low_verts, (int)low_num_verts, low_faces, low_normals, max_dist, tr, normals, owner, normal_map, dist, hit_face);
    return check_launch("v3d_recon_tex_bake_normals");
}
