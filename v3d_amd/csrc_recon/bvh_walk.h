// Shared by the sources of libv3d_recon.so that walk the tree of include/v3d_recon.h "THE NODES" (meshbvh.hip, meshquery.hip): the tree's
// arguments, the ray, the box and triangle tests, the closest-hit walk and its LDS stack convention (stack[entry * 64 + lane], the calling
// lane's column handed in as `stack + lane`), and the host helpers behind the entries that take a tree.  Moved here from meshbvh.hip, whose
// head comment says why the stack lives in LDS and why a block is one wave.  Everything sits in an anonymous namespace: every source that
// includes this gets its own copy, as when the code stood in the source itself.
#ifndef V3D_RECON_BVH_WALK_H
#define V3D_RECON_BVH_WALK_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "recon_host.h"
#include "v3d_recon.h"

namespace {

constexpr int BT = 64;                         // threads to a block of the traversal kernels: one wave
constexpr int STACK = V3D_RECON_BVH_STACK;     // entries; the height is at most 30 + bits(F - 1) <= 61
constexpr float BOX_SLACK = 3.814697265625e-6f;          // 2^-18: the box interval is widened by this share of |t| on both ends

struct Tree {
    const int32_t *left, *right, *order;
    const float *lo, *hi, *verts;
    const int32_t* faces;
    int nv, nf;
};

__device__ __forceinline__ bool vert_ok(int v, int nv) { return v >= 0 && v < nv; }

// ---------------------------------------------------------------------------------------------------------------------------------------
// Closest hit.
struct Ray {
    float ox, oy, oz, dx, dy, dz, ix, iy, iz;
};

struct Hit {
    float t, u, v;
    int face;
};

__device__ __forceinline__ Ray make_ray(float ox, float oy, float oz, float dx, float dy, float dz) {
    return Ray{ox, oy, oz, dx, dy, dz, 1.f / dx, 1.f / dy, 1.f / dz};
}

__device__ __forceinline__ void slab(float lo, float hi, float o, float inv, float& tn, float& tf) {
    const float t0 = (lo - o) * inv, t1 = (hi - o) * inv;
    // 0 x inf: a zero direction component with the origin on one of the slab's planes.  The ray runs inside the slab: no constraint.
    if (t0 != t0 || t1 != t1) return;
    tn = fmaxf(tn, fminf(t0, t1));
    tf = fminf(tf, fmaxf(t0, t1));
}

// Conservative: true for every box the ray enters at some t in [tmin, best], and for some it misses.  `entry` orders the children.
__device__ __forceinline__ bool enters(const Tree& tr, int node, const Ray& r, float tmin, float best, float& entry) {
    const float* lo = tr.lo + 3 * (long long)node;
    const float* hi = tr.hi + 3 * (long long)node;
    float tn = -INFINITY, tf = INFINITY;
    slab(lo[0], hi[0], r.ox, r.ix, tn, tf);
    slab(lo[1], hi[1], r.oy, r.iy, tn, tf);
    slab(lo[2], hi[2], r.oz, r.iz, tn, tf);
    entry = tn - fabsf(tn) * BOX_SLACK;
    const float exit = tf + fabsf(tf) * BOX_SLACK;
    return entry <= exit && entry <= best && exit >= tmin;
}

// Moeller-Trumbore on e1 = v1 - v0, e2 = v2 - v0.  cull: 0 every triangle, 1 only Ng . d < 0, 2 only Ng . d > 0, Ng = e1 x e2.
// open_min: t > tmin in the place of t >= tmin.
__device__ __forceinline__ void hit_triangle(const Tree& tr, int face, const Ray& r, float tmin, float tmax, int cull, bool open_min, Hit& best) {
    if (face < 0 || face >= tr.nf) return;
    const int i0 = tr.faces[3 * (long long)face], i1 = tr.faces[3 * (long long)face + 1], i2 = tr.faces[3 * (long long)face + 2];
    if (!(vert_ok(i0, tr.nv) && vert_ok(i1, tr.nv) && vert_ok(i2, tr.nv))) return;
    const float* a = tr.verts + 3 * (long long)i0;
    const float* b = tr.verts + 3 * (long long)i1;
    const float* c = tr.verts + 3 * (long long)i2;
    const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    if (cull) {
        const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        const float nd = nx * r.dx + ny * r.dy + nz * r.dz;
        if (cull == 1 ? !(nd < 0.f) : !(nd > 0.f)) return;
    }
    const float px = r.dy * e2z - r.dz * e2y, py = r.dz * e2x - r.dx * e2z, pz = r.dx * e2y - r.dy * e2x;
    const float det = e1x * px + e1y * py + e1z * pz;
    if (det == 0.f) return;
    const float inv = 1.f / det;
    const float sx = r.ox - a[0], sy = r.oy - a[1], sz = r.oz - a[2];
    const float u = (sx * px + sy * py + sz * pz) * inv;
    const float qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;
    const float v = (r.dx * qx + r.dy * qy + r.dz * qz) * inv;
    const float t = (e2x * qx + e2y * qy + e2z * qz) * inv;
    if (!(u >= 0.f && v >= 0.f && u + v <= 1.f)) return;
    if (!((open_min ? t > tmin : t >= tmin) && t <= tmax)) return;
    if (t < best.t || (t == best.t && face < best.face)) best = Hit{t, u, v, face};
}

// The walk.  `stack` is the calling lane's column of the block's LDS stack: entry k at stack[k * BT].  One child is pushed and the other
// descended, so the depth never exceeds the tree's height; a push beyond STACK or a walk longer than the tree has nodes (neither can
// happen on a tree of build_nodes) is dropped rather than followed.
__device__ Hit closest_hit(const Tree& tr, const Ray& r, float tmin, float tmax, int cull, bool open_min, int* stack) {
    Hit best{INFINITY, 0.f, 0.f, -1};
    const int inner = tr.nf - 1, nodes = 2 * tr.nf - 1;
    float e;
    if (!enters(tr, 0, r, tmin, tmax, e)) return best;
    int sp = 0, node = 0;
    for (int step = 0; step < nodes; ++step) {
        bool pop = true;
        if (node >= inner) {
            const uint32_t f = tr.order[node - inner];
            hit_triangle(tr, f < (uint32_t)tr.nf ? (int)f : -1, r, tmin, tmax, cull, open_min, best);
        } else {
            const int a = tr.left[node], b = tr.right[node];
            float ea, eb;
            const float far = fminf(best.t, tmax);
            const bool ha = a >= 0 && a < nodes && enters(tr, a, r, tmin, far, ea);
            const bool hb = b >= 0 && b < nodes && enters(tr, b, r, tmin, far, eb);
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
    return best;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// What the kernels over the atlas share.
__device__ __forceinline__ bool unit(float& x, float& y, float& z) {
    const float len2 = x * x + y * y + z * z;
    if (len2 > 1e-20f) {
        const float len = sqrtf(len2);
        x /= len;
        y /= len;
        z /= len;
        return true;
    }
    x = 0.f, y = 0.f, z = 1.f;                     // the rule of mesh_vertex_normals
    return false;
}

// g = ceil(sqrt(ceil(F / 2))), S = floor(R / g) (meshtex.hip's atlas_of)
bool atlas_cells(int32_t F, int32_t R, int* S, int* g) {
    const long long cells = ((long long)F + 1) / 2;
    long long gg = (long long)ceil(sqrt((double)cells));
    while (gg * gg < cells) ++gg;
    while (gg > 1 && (gg - 1) * (gg - 1) >= cells) --gg;
    *g = (int)gg, *S = (int)(R / gg);
    return *S >= V3D_RECON_TEX_MIN_CELL;
}

unsigned nblk_bt(long long n) { return (unsigned)((n + BT - 1) / BT); }

}  // namespace

#define ST ((hipStream_t)stream)
#define BVH_MAX_FACES (1 << 30)                    /* 2 F - 1 fits int32 */
#define BVH_REQUIRE_FACES(name, F) \
    RECON_REQUIRE((F) > 0 && (F) <= BVH_MAX_FACES, name ": num_faces %d outside 1 .. %d", (int)(F), BVH_MAX_FACES)
#define BVH_REQUIRE_TREE(name, left, right, order, lo, hi, verts, nv, faces, F)                                                   \
    RECON_REQUIRE((left) && (right) && (order) && (lo) && (hi) && (verts) && (faces), name ": null argument");                   \
    RECON_REQUIRE((nv) > 0, name ": num_verts must be positive");                                                               \
    BVH_REQUIRE_FACES(name, F)

#endif
