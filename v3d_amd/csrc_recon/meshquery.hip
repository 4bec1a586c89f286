// More queries on the tree of meshbvh.hip (include/v3d_recon.h "Mesh queries", libv3d_recon.so; host side: v3d_amd/recon/mesh_query.py):
// closest_point (a walk ordered by the distance to a node's box; with face_samples, the midpoint quadrature, the distance between two
// meshes), occlusion (a walk that stops at the first hit, a hemisphere of rays per point; with tex_texel_frames an ambient-occlusion map on
// the atlas of meshtex.hip).  The tree, the ray tests, the closest-point walk (shared with meshsolid.hip) and the stack convention are
// bvh_walk.h's.
//
// No atomics.  closest_point's result is the smallest d2 over the triangle tests and, on equal d2, the smaller face: a function of the set
// of triangles tested; a node is left out only when its box lies further than the best by more than the slack, so in exact arithmetic the
// set holds every triangle that could win.  In float a triangle's d2 carries the rounding of q = a + u e1 + v e2, a few ulps of the
// COORDINATES: for a query much nearer to the surface than the coordinates are large that can exceed the slack, and a leaf whose computed
// d2 would have tied or won by less than that error can be skipped.  The answer stays a function of the arguments and within that
// rounding of the smallest distance (the header says the same).  occlusion's result is a boolean of the set of triangles, so the order of the walk cannot change it; a
// point's count comes from a ballot over its own wave and is written by lane 0.
//
// The stacks live in LDS as in meshbvh.hip: 16 KB to a block of one wave, so 10 waves to a CU.  stack[entry * 64 + lane] puts lane l on
// bank l mod 32 whatever its depth, and the two halves of a wave are served in turn: no conflicts however far the lanes have diverged.
// occlusion gives a whole wave to a point: with fewer than 64 samples the other lanes idle (a known cost; points are not packed into a wave).
// Built without -ffast-math (v3d_amd/build.py): everything is held to an fp64 restatement (tests/mesh_query_ref.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "bvh_walk.h"
#include "recon_host.h"
#include "v3d_recon.h"

namespace {

__global__ void __launch_bounds__(BT) bvh_closest_point_kernel(Tree tr, const float* __restrict__ points, int n, float max_d2, float* __restrict__ dist,
                                                               int32_t* __restrict__ face, float* __restrict__ uv) {
    __shared__ int stack[STACK * BT];
    const long long i = (long long)blockIdx.x * BT + threadIdx.x;
    if (i >= n) return;
    const float px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
    Near h{INFINITY, 0.f, 0.f, -1};
    if (isfinite(px) && isfinite(py) && isfinite(pz)) h = closest_point(tr, px, py, pz, max_d2, stack + threadIdx.x);
    const bool found = h.face >= 0;
    dist[i] = found ? sqrtf(h.d2) : INFINITY;
    face[i] = found ? h.face : -1;
    uv[2 * i] = found ? h.u : 0.f;
    uv[2 * i + 1] = found ? h.v : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Samples.
__global__ void __launch_bounds__(NT) mesh_face_samples_kernel(const float* __restrict__ verts, int nv, const int32_t* __restrict__ faces, int nf, int n,
                                                               float* __restrict__ points, float* __restrict__ weights) {
    const long long s = (long long)blockIdx.x * NT + threadIdx.x;
    const int n2 = n * n;
    if (s >= (long long)nf * n2) return;
    const long long f = s / n2;
    int k = (int)(s - f * n2);
    const int up = n * (n + 1) / 2;
    float t = 1.f / 3.f;
    int rows = n;
    if (k >= up) k -= up, t = 2.f / 3.f, rows = n - 1;
    int j = 0;
    while (k >= rows - j) k -= rows - j, ++j;       // row j holds rows - j sub-triangles; k is left as i
    const float b1 = ((float)k + t) / (float)n, b2 = ((float)j + t) / (float)n;
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    float x = 0.f, y = 0.f, z = 0.f, w = 0.f;
    if (vert_ok(i0, nv) && vert_ok(i1, nv) && vert_ok(i2, nv)) {
        const float* a = verts + 3 * (long long)i0;
        const float* b = verts + 3 * (long long)i1;
        const float* c = verts + 3 * (long long)i2;
        const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
        const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
        const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        x = a[0] + b1 * e1x + b2 * e2x, y = a[1] + b1 * e1y + b2 * e2y, z = a[2] + b1 * e1z + b2 * e2z;
        w = 0.5f * sqrtf(dot3(nx, ny, nz, nx, ny, nz)) / (float)n2;
    }
    points[3 * s] = x;
    points[3 * s + 1] = y;
    points[3 * s + 2] = z;
    weights[s] = w;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Occlusion.  The walk of closest_hit that returns at the first triangle hit; the box test keeps best = tmax throughout.
__device__ bool any_hit(const Tree& tr, const Ray& r, float tmin, float tmax, int* stack) {
    const int inner = tr.nf - 1, nodes = 2 * tr.nf - 1;
    float e;
    if (!enters(tr, 0, r, tmin, tmax, e)) return false;
    int sp = 0, node = 0;
    for (int step = 0; step < nodes; ++step) {
        bool pop = true;
        if (node >= inner) {
            const uint32_t f = tr.order[node - inner];
            Hit h{INFINITY, 0.f, 0.f, -1};
            hit_triangle(tr, f < (uint32_t)tr.nf ? (int)f : -1, r, tmin, tmax, 0, false, h);
            if (h.face >= 0) return true;
        } else {
            const int a = tr.left[node], b = tr.right[node];
            float ea, eb;
            const bool ha = a >= 0 && a < nodes && enters(tr, a, r, tmin, tmax, ea);
            const bool hb = b >= 0 && b < nodes && enters(tr, b, r, tmin, tmax, eb);
            if (ha && hb) {
                const bool a_first = ea <= eb;
                if (sp < STACK) stack[BT * sp++] = a_first ? b : a;
                node = a_first ? a : b;
                pop = false;
            } else if (ha || hb) {
                node = ha ? a : b;
                pop = false;
            }
        }
        if (pop) {
            if (sp == 0) break;
            node = stack[BT * --sp];
        }
    }
    return false;
}

__global__ void __launch_bounds__(BT) bvh_occlusion_kernel(Tree tr, const float* __restrict__ points, const float* __restrict__ normals, int K, float radius,
                                                           float bias, uint32_t seed, int32_t* __restrict__ hits) {
    __shared__ int stack[STACK * BT];
    const long long i = blockIdx.x;
    const int lane = threadIdx.x;
    const float px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
    float nx = normals[3 * i], ny = normals[3 * i + 1], nz = normals[3 * i + 2];
    const float len2 = nx * nx + ny * ny + nz * nz;
    if (!(isfinite(px) && isfinite(py) && isfinite(pz)) || !(len2 > 1e-20f) || !isfinite(len2)) {          // (the same for every lane)
        if (lane == 0) hits[i] = -1;
        return;
    }
    unit(nx, ny, nz);
    uint32_t h = (((uint32_t)i + 1u) * 0x9E3779B9u) ^ seed;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    const float s = copysignf(1.f, nz), a = -1.f / (s + nz), b = nx * ny * a;
    const float t1x = 1.f + s * nx * nx * a, t1y = s * b, t1z = -s * nx;
    const float t2x = b, t2y = s + ny * ny * a, t2z = -ny;
    const float ox = px + bias * nx, oy = py + bias * ny, oz = pz + bias * nz;
    int count = 0;
    for (int base = 0; base < K; base += BT) {     // every lane runs every round: the ballot needs the whole wave
        const int k = base + lane;
        bool hit = false;
        if (k < K) {
            const float frac = (float)((uint32_t)k * 2654435769u + h) * 2.3283064365386963e-10f;          // / 2^32
            const float u = ((float)k + 0.5f) / (float)K;
            const float r = sqrtf(u), z = sqrtf(1.f - u);
            float sn, cs;
            sincospif(2.f * frac, &sn, &cs);
            const float dx = r * cs * t1x + r * sn * t2x + z * nx, dy = r * cs * t1y + r * sn * t2y + z * ny, dz = r * cs * t1z + r * sn * t2z + z * nz;
            hit = any_hit(tr, make_ray(ox, oy, oz, dx, dy, dz), 0.f, radius, stack + lane);
        }
        count += __popcll(__ballot(hit));
    }
    if (lane == 0) hits[i] = count;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The frames of the atlas.  The atlas arithmetic is meshbvh.hip's tex_bake_normals_kernel, statement for statement.
__global__ void __launch_bounds__(NT) tex_texel_frames_kernel(int R, int S, int g, int F, const float* __restrict__ lverts, int lnv,
                                                              const int32_t* __restrict__ lfaces, const float* __restrict__ lnormals,
                                                              int32_t* __restrict__ owner, float* __restrict__ pos, float* __restrict__ nrm) {
    const long long t = (long long)blockIdx.x * NT + threadIdx.x;
    if (t >= (long long)R * R) return;
    const int x = (int)(t % R), y = (int)(t / R);
    int f = -1;
    float n0 = 0.f, n1 = 0.f, n2 = 1.f, px = NAN, py = NAN, pz = NAN;
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
                px = b0 * p0[0] + b1 * p1[0] + b2 * p2[0], py = b0 * p0[1] + b1 * p1[1] + b2 * p2[1], pz = b0 * p0[2] + b1 * p1[2] + b2 * p2[2];
                n0 = b0 * m0[0] + b1 * m1[0] + b2 * m2[0];
                n1 = b0 * m0[1] + b1 * m1[1] + b2 * m2[1];
                n2 = b0 * m0[2] + b1 * m1[2] + b2 * m2[2];
                unit(n0, n1, n2);
            }
        }
    }
    owner[t] = f;
    pos[3 * t] = px;
    pos[3 * t + 1] = py;
    pos[3 * t + 2] = pz;
    nrm[3 * t] = n0;
    nrm[3 * t + 1] = n1;
    nrm[3 * t + 2] = n2;
}

}  // namespace

extern "C" int v3d_recon_bvh_closest_point(const float* points, int32_t num_points, float max_dist, const int32_t* left, const int32_t* right,
                                           const uint32_t* order, const float* lo, const float* hi, const float* verts, int32_t num_verts,
                                           const int32_t* faces, int32_t num_faces, float* dist, int32_t* face, float* uv, v3d_stream_t stream) {
    RECON_REQUIRE(points && dist && face && uv, "v3d_recon_bvh_closest_point: null argument");
    BVH_REQUIRE_TREE("v3d_recon_bvh_closest_point", left, right, order, lo, hi, verts, num_verts, faces, num_faces);
    RECON_REQUIRE(num_points > 0, "v3d_recon_bvh_closest_point: num_points must be positive");
    RECON_REQUIRE(max_dist >= 0.f, "v3d_recon_bvh_closest_point: max_dist %g must not be negative or NaN", (double)max_dist);
    const Tree tr{left, right, (const int32_t*)order, lo, hi, verts, faces, (int)num_verts, (int)num_faces};
    hipLaunchKernelGGL(bvh_closest_point_kernel, dim3(nblk_bt(num_points)), dim3(BT), 0, ST, tr, points, (int)num_points, max_dist * max_dist, dist, face,
                       uv);
    return check_launch("v3d_recon_bvh_closest_point");
}

extern "C" int v3d_recon_mesh_face_samples(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, int32_t subdivide, float* points,
                                           float* weights, v3d_stream_t stream) {
    RECON_REQUIRE(verts && faces && points && weights, "v3d_recon_mesh_face_samples: null argument");
    RECON_REQUIRE(num_verts > 0, "v3d_recon_mesh_face_samples: num_verts must be positive");
    RECON_REQUIRE(num_faces > 0, "v3d_recon_mesh_face_samples: num_faces must be positive");
    RECON_REQUIRE(subdivide >= 1 && subdivide <= V3D_RECON_SAMPLES_MAX_SUBDIVIDE, "v3d_recon_mesh_face_samples: subdivide %d outside 1 .. %d", (int)subdivide,
                  V3D_RECON_SAMPLES_MAX_SUBDIVIDE);
    const long long total = (long long)num_faces * subdivide * subdivide;
    RECON_REQUIRE(total <= INT32_MAX, "v3d_recon_mesh_face_samples: %lld samples do not fit int32", total);
    hipLaunchKernelGGL(mesh_face_samples_kernel, dim3(nblk(total)), dim3(NT), 0, ST, verts, (int)num_verts, faces, (int)num_faces, (int)subdivide, points,
                       weights);
    return check_launch("v3d_recon_mesh_face_samples");
}

extern "C" int v3d_recon_bvh_occlusion(const float* points, const float* normals, int32_t num_points, int32_t num_samples, float radius, float bias,
                                       uint32_t seed, const int32_t* left, const int32_t* right, const uint32_t* order, const float* lo, const float* hi,
                                       const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, int32_t* hits, v3d_stream_t stream) {
    RECON_REQUIRE(points && normals && hits, "v3d_recon_bvh_occlusion: null argument");
    BVH_REQUIRE_TREE("v3d_recon_bvh_occlusion", left, right, order, lo, hi, verts, num_verts, faces, num_faces);
    RECON_REQUIRE(num_points > 0, "v3d_recon_bvh_occlusion: num_points must be positive");
    RECON_REQUIRE(num_samples >= 1 && num_samples <= V3D_RECON_OCCLUSION_MAX_SAMPLES, "v3d_recon_bvh_occlusion: num_samples %d outside 1 .. %d",
                  (int)num_samples, V3D_RECON_OCCLUSION_MAX_SAMPLES);
    RECON_REQUIRE(radius > 0.f && isfinite(radius), "v3d_recon_bvh_occlusion: radius %g must be finite and positive", (double)radius);
    RECON_REQUIRE(bias >= 0.f && isfinite(bias), "v3d_recon_bvh_occlusion: bias %g must be finite and not negative", (double)bias);
    const Tree tr{left, right, (const int32_t*)order, lo, hi, verts, faces, (int)num_verts, (int)num_faces};
    hipLaunchKernelGGL(bvh_occlusion_kernel, dim3((unsigned)num_points), dim3(BT), 0, ST, tr, points, normals, (int)num_samples, radius, bias, seed, hits);
    return check_launch("v3d_recon_bvh_occlusion");
}

extern "C" int v3d_recon_tex_texel_frames(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const float* normals,
                                          int32_t tex_size, int32_t* owner, float* positions, float* frame_normals, v3d_stream_t stream) {
    RECON_REQUIRE(verts && faces && normals && owner && positions && frame_normals, "v3d_recon_tex_texel_frames: null argument");
    RECON_REQUIRE(num_verts > 0, "v3d_recon_tex_texel_frames: num_verts must be positive");
    RECON_REQUIRE(num_faces > 0, "v3d_recon_tex_texel_frames: num_faces must be positive");
    RECON_REQUIRE(tex_size >= 1 && tex_size <= V3D_RECON_TEX_MAX_SIZE, "v3d_recon_tex_texel_frames: tex_size %d outside 1 .. %d", (int)tex_size,
                  V3D_RECON_TEX_MAX_SIZE);
    int S, g;
    RECON_REQUIRE(atlas_cells(num_faces, tex_size, &S, &g), "v3d_recon_tex_texel_frames: texture too small for %d faces: %d x %d leaves cells of %d texels, below %d",
                  (int)num_faces, (int)tex_size, (int)tex_size, S, V3D_RECON_TEX_MIN_CELL);
    hipLaunchKernelGGL(tex_texel_frames_kernel, dim3(nblk((long long)tex_size * tex_size)), dim3(NT), 0, ST, (int)tex_size, S, g, (int)num_faces, verts,
                       (int)num_verts, faces, normals, owner, positions, frame_normals);
    return check_launch("v3d_recon_tex_texel_frames");
}
