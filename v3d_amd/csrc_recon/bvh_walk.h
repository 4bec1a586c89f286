// Shared by the sources of libv3d_recon.so that walk the tree of include/v3d_recon.h "THE NODES" (meshbvh.hip, meshquery.hip, meshsolid.hip):
// the tree's arguments, the ray, the box and triangle tests, the closest-hit walk, the closest-point walk (region method and bounded descent)
// and their LDS stack convention (stack[entry * 64 + lane], the calling
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
// Closest point.  Moved here from meshquery.hip without a changed statement, for meshsolid.hip to share.
constexpr float NEAR_SLACK = 3.814697265625e-6f;         // 2^-18: a node is skipped only when bound (1 - 2^-18) > best d2

struct Near {
    float d2, u, v;
    int face;
};

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// The squared distance from p to the node's box; +inf for the empty box of a face that is never returned.
__device__ __forceinline__ float box_d2(const Tree& tr, int node, float px, float py, float pz) {
    const float* lo = tr.lo + 3 * (long long)node;
    const float* hi = tr.hi + 3 * (long long)node;
    const float dx = px - fminf(fmaxf(px, lo[0]), hi[0]), dy = py - fminf(fmaxf(py, lo[1]), hi[1]), dz = pz - fminf(fmaxf(pz, lo[2]), hi[2]);
    return dot3(dx, dy, dz, dx, dy, dz);
}

__device__ __forceinline__ bool beyond(float bound, float best) { return bound * (1.f - NEAR_SLACK) > best; }

// e1 x e2 == 0 with every product rounded on its own.  Written as comparisons of products: a difference a b - b a would be fused (the
// library is built with contraction on) and leave the rounding error of one product, and a face with two equal corners must give exactly 0.
__device__ __forceinline__ bool no_area(float e1x, float e1y, float e1z, float e2x, float e2y, float e2z) {
    return e1y * e2z == e1z * e2y && e1z * e2x == e1x * e2z && e1x * e2y == e1y * e2x;
}

// THE CLOSEST POINT OF A TRIANGLE of the header, statement by statement.
__device__ __forceinline__ void near_triangle(const Tree& tr, int face, float px, float py, float pz, Near& best) {
    if (face < 0 || face >= tr.nf) return;
    const int i0 = tr.faces[3 * (long long)face], i1 = tr.faces[3 * (long long)face + 1], i2 = tr.faces[3 * (long long)face + 2];
    if (!(vert_ok(i0, tr.nv) && vert_ok(i1, tr.nv) && vert_ok(i2, tr.nv))) return;
    const float* a = tr.verts + 3 * (long long)i0;
    const float* b = tr.verts + 3 * (long long)i1;
    const float* c = tr.verts + 3 * (long long)i2;
    const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    if (no_area(e1x, e1y, e1z, e2x, e2y, e2z)) return;
    float u, v;
    const float d1 = dot3(e1x, e1y, e1z, px - a[0], py - a[1], pz - a[2]), d2 = dot3(e2x, e2y, e2z, px - a[0], py - a[1], pz - a[2]);
    const float d3 = dot3(e1x, e1y, e1z, px - b[0], py - b[1], pz - b[2]), d4 = dot3(e2x, e2y, e2z, px - b[0], py - b[1], pz - b[2]);
    const float d5 = dot3(e1x, e1y, e1z, px - c[0], py - c[1], pz - c[2]), d6 = dot3(e2x, e2y, e2z, px - c[0], py - c[1], pz - c[2]);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float m = d4 - d3, n = d5 - d6;
    if (d1 <= 0.f && d2 <= 0.f) {
        u = 0.f, v = 0.f;
    } else if (d3 >= 0.f && d4 <= d3) {
        u = 1.f, v = 0.f;
    } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
        u = d1 / (d1 - d3), v = 0.f;
    } else if (d6 >= 0.f && d5 <= d6) {
        u = 0.f, v = 1.f;
    } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
        u = 0.f, v = d2 / (d2 - d6);
    } else if (va <= 0.f && m >= 0.f && n >= 0.f) {
        const float w = m / (m + n);
        u = 1.f - w, v = w;
    } else {
        const float s = va + vb + vc;
        u = vb / s, v = vc / s;
    }
    float qx = a[0] + u * e1x + v * e2x, qy = a[1] + u * e1y + v * e2y, qz = a[2] + u * e1z + v * e2z;
    if (u == 1.f) qx = b[0], qy = b[1], qz = b[2];             // a vertex is itself, not a + (b - a) rounded twice: a query at a vertex is 0 away
    if (v == 1.f) qx = c[0], qy = c[1], qz = c[2];
    const float rx = px - qx, ry = py - qy, rz = pz - qz;
    const float dd = dot3(rx, ry, rz, rx, ry, rz);
    if (!(dd < INFINITY)) return;                  // a sliver whose sums underflowed (u = 0 / 0), or an overflow: never an answer
    // closed at the start value: best.face < 0 means nothing found yet, and d2 == max_dist^2 is found
    if (dd < best.d2 || (dd == best.d2 && (best.face < 0 || face < best.face))) best = Near{dd, u, v, face};
}

// The walk of closest_hit with the bound in the place of the box test: the nearer child is descended, the other pushed.
__device__ Near closest_point(const Tree& tr, float px, float py, float pz, float max_d2, int* stack) {
    Near best{max_d2, 0.f, 0.f, -1};
    const int inner = tr.nf - 1, nodes = 2 * tr.nf - 1;
    if (beyond(box_d2(tr, 0, px, py, pz), best.d2)) return best;
    int sp = 0, node = 0;
    for (int step = 0; step < nodes; ++step) {
        bool pop = true;
        if (beyond(box_d2(tr, node, px, py, pz), best.d2)) {
            // (pushed when the best was still further away)
        } else if (node >= inner) {
            const uint32_t f = tr.order[node - inner];
            near_triangle(tr, f < (uint32_t)tr.nf ? (int)f : -1, px, py, pz, best);
        } else {
            const int a = tr.left[node], b = tr.right[node];
            const bool oa = a >= 0 && a < nodes, ob = b >= 0 && b < nodes;
            const float da = oa ? box_d2(tr, a, px, py, pz) : INFINITY, db = ob ? box_d2(tr, b, px, py, pz) : INFINITY;
            const bool ha = oa && !beyond(da, best.d2), hb = ob && !beyond(db, best.d2);
            if (ha && hb) {
                const bool a_first = da <= db;
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
