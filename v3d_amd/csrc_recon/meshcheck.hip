// Is the mesh sound (include/v3d_recon.h "Mesh check", libv3d_recon.so; host side: v3d_amd/recon/mesh_check.py): which pairs of faces pass
// through each other, and how many faces meet at every edge and which way they run.  bvh_self_count / bvh_self_emit walk the tree of
// meshbvh.hip with the mesh's own faces as queries (bvh_walk.h: the tree's arguments, no_area, the LDS stack convention; meshbvh.hip's head
// comment says why the stack lives in LDS and why a block is one wave); mesh_edge_census / mesh_vertex_census walk the vertex -> corner lists
// of mesh_lists.h (struct Lists, closed_fan).
//
// No atomics.  A pair (f, g) is decided by one function of the two faces, always called with the lower-indexed face first, so lane f and
// lane g decide alike and n_all is symmetric; the walk only ever leaves out faces whose exact box misses f's, which the pair rule refuses
// anyway, so the set of partners does not depend on the tree's shape.  count and emit run the same walk: emit's j-th partner g > f is
// count's j-th.  Two runs are bit-equal.
//
// Lane i of the launch takes face order[i], the i-th leaf: neighbouring lanes then hold neighbouring boxes and descend the same nodes for
// most of their walk.  The walk pushes the right child and descends the left; nothing orders them, every overlapping node is visited.
// Built without -ffast-math (v3d_amd/build.py) and, from the pragma on, without contraction: every product below is rounded on its own, as
// the float32 run of the restatement (tests/mesh_check_ref.py) rounds it.  (no_area of bvh_walk.h compares products and has nothing to fuse.)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "bvh_walk.h"
#include "mesh_lists.h"
#include "recon_host.h"
#include "v3d_recon.h"

#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------------------------------------------------------------------------------
// THE PAIR RULE of the header, statement by statement.
struct Tri {
    int i0, i1, i2;
    float ax, ay, az, bx, by, bz, cx, cy, cz;
    float lox, loy, loz, hix, hiy, hiz;
};

// (a): the face is present and has area; its box is the min and max of its three vertices
__device__ __forceinline__ bool load_tri(const Tree& tr, int face, Tri& t) {
    if (face < 0 || face >= tr.nf) return false;
    t.i0 = tr.faces[3 * (long long)face], t.i1 = tr.faces[3 * (long long)face + 1], t.i2 = tr.faces[3 * (long long)face + 2];
    if (!(vert_ok(t.i0, tr.nv) && vert_ok(t.i1, tr.nv) && vert_ok(t.i2, tr.nv))) return false;
    const float* a = tr.verts + 3 * (long long)t.i0;
    const float* b = tr.verts + 3 * (long long)t.i1;
    const float* c = tr.verts + 3 * (long long)t.i2;
    t.ax = a[0], t.ay = a[1], t.az = a[2];
    t.bx = b[0], t.by = b[1], t.bz = b[2];
    t.cx = c[0], t.cy = c[1], t.cz = c[2];
    if (no_area(t.bx - t.ax, t.by - t.ay, t.bz - t.az, t.cx - t.ax, t.cy - t.ay, t.cz - t.az)) return false;
    t.lox = fminf(t.ax, fminf(t.bx, t.cx)), t.loy = fminf(t.ay, fminf(t.by, t.cy)), t.loz = fminf(t.az, fminf(t.bz, t.cz));
    t.hix = fmaxf(t.ax, fmaxf(t.bx, t.cx)), t.hiy = fmaxf(t.ay, fmaxf(t.by, t.cy)), t.hiz = fmaxf(t.az, fmaxf(t.bz, t.cz));
    return true;
}

__device__ __forceinline__ float dotp(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// x component of u x w; the others by rotating the arguments
__device__ __forceinline__ float cross1(float uy, float uz, float wy, float wz) { return uy * wz - uz * wy; }

// d . (u x w)
__device__ __forceinline__ float triple(float dx, float dy, float dz, float ux, float uy, float uz, float wx, float wy, float wz) {
    return dotp(dx, dy, dz, cross1(uy, uz, wy, wz), cross1(uz, ux, wz, wx), cross1(ux, uy, wx, wy));
}

// (d): the edge (p, q) against the triangle (a, b, c)
__device__ __forceinline__ bool edge_crosses(float px, float py, float pz, float qx, float qy, float qz, float ax, float ay, float az, float bx, float by,
                                             float bz, float cx, float cy, float cz) {
    const float e1x = bx - ax, e1y = by - ay, e1z = bz - az;
    const float e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
    const float nx = cross1(e1y, e1z, e2y, e2z), ny = cross1(e1z, e1x, e2z, e2x), nz = cross1(e1x, e1y, e2x, e2y);
    const float dp = dotp(nx, ny, nz, px - ax, py - ay, pz - az);
    const float dq = dotp(nx, ny, nz, qx - ax, qy - ay, qz - az);
    if (!((dp > 0.f && dq < 0.f) || (dp < 0.f && dq > 0.f))) return false;
    const float dx = qx - px, dy = qy - py, dz = qz - pz;
    const float apx = ax - px, apy = ay - py, apz = az - pz;
    const float bpx = bx - px, bpy = by - py, bpz = bz - pz;
    const float cpx = cx - px, cpy = cy - py, cpz = cz - pz;
    const float ta = triple(dx, dy, dz, bpx, bpy, bpz, cpx, cpy, cpz);
    const float tb = triple(dx, dy, dz, cpx, cpy, cpz, apx, apy, apz);
    const float tc = triple(dx, dy, dz, apx, apy, apz, bpx, bpy, bpz);
    return dp > 0.f ? (ta <= 0.f && tb <= 0.f && tc <= 0.f) : (ta >= 0.f && tb >= 0.f && tc >= 0.f);
}

// corner k of t
__device__ __forceinline__ void corner_of(const Tri& t, int k, float& x, float& y, float& z) {
    x = k == 0 ? t.ax : (k == 1 ? t.bx : t.cx);
    y = k == 0 ? t.ay : (k == 1 ? t.by : t.cy);
    z = k == 0 ? t.az : (k == 1 ? t.bz : t.cz);
}

// the edge of e from corner k to corner (k + 1) % 3 against the triangle t
__device__ __forceinline__ bool edge_of(const Tri& e, int k, const Tri& t) {
    float px, py, pz, qx, qy, qz;
    corner_of(e, k, px, py, pz);
    corner_of(e, (k + 1) % 3, qx, qy, qz);
    return edge_crosses(px, py, pz, qx, qy, qz, t.ax, t.ay, t.az, t.bx, t.by, t.bz, t.cx, t.cy, t.cz);
}

// (b), (c), (d) for two faces that passed (a); A is the face of the lower index
__device__ bool pair_crosses(const Tri& A, const Tri& B) {
    if (!(A.lox <= B.hix && B.lox <= A.hix && A.loy <= B.hiy && B.loy <= A.hiy && A.loz <= B.hiz && B.loz <= A.hiz)) return false;
    const int a0 = (A.i0 == B.i0) + (A.i0 == B.i1) + (A.i0 == B.i2);
    const int a1 = (A.i1 == B.i0) + (A.i1 == B.i1) + (A.i1 == B.i2);
    const int a2 = (A.i2 == B.i0) + (A.i2 == B.i1) + (A.i2 == B.i2);
    const int s = a0 + a1 + a2;
    if (s >= 2) return false;
    if (s == 1) {
        const int ka = a0 ? 0 : (a1 ? 1 : 2);                 // the shared vertex's corner in A, and in B
        const int sv = ka == 0 ? A.i0 : (ka == 1 ? A.i1 : A.i2);
        const int kb = B.i0 == sv ? 0 : (B.i1 == sv ? 1 : 2);
        return edge_of(A, (ka + 1) % 3, B) || edge_of(B, (kb + 1) % 3, A);
    }
    return edge_of(A, 0, B) || edge_of(A, 1, B) || edge_of(A, 2, B) || edge_of(B, 0, A) || edge_of(B, 1, A) || edge_of(B, 2, A);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The walk of closest_hit with the closed overlap of two boxes in the place of the ray test: the left child is descended, the right pushed.
__device__ __forceinline__ bool meets(const Tree& tr, int node, const Tri& t) {
    const float* lo = tr.lo + 3 * (long long)node;
    const float* hi = tr.hi + 3 * (long long)node;
    return t.lox <= hi[0] && lo[0] <= t.hix && t.loy <= hi[1] && lo[1] <= t.hiy && t.loz <= hi[2] && lo[2] <= t.hiz;
}

// EMIT: partner j (counted over g > f in walk order) goes to pairs[first + j] while first + j < last
template <bool EMIT>
__device__ void self_walk(const Tree& tr, int f, const Tri& mine, int* stack, int& n_all, int& n_up, int32_t* __restrict__ pairs, long long first,
                          long long last) {
    n_all = 0, n_up = 0;
    const int inner = tr.nf - 1, nodes = 2 * tr.nf - 1;
    if (!meets(tr, 0, mine)) return;
    int sp = 0, node = 0;
    for (int step = 0; step < nodes; ++step) {
        bool pop = true;
        if (node >= inner) {
            const uint32_t gu = tr.order[node - inner];
            const int g = gu < (uint32_t)tr.nf ? (int)gu : -1;
            Tri other;
            if (g >= 0 && g != f && load_tri(tr, g, other) && (f < g ? pair_crosses(mine, other) : pair_crosses(other, mine))) {
                ++n_all;
                if (g > f) {
                    if (EMIT && first + n_up < last) {
                        pairs[2 * (first + n_up)] = f;
                        pairs[2 * (first + n_up) + 1] = g;
                    }
                    ++n_up;
                }
            }
        } else {
            const int a = tr.left[node], b = tr.right[node];
            const bool ha = a >= 0 && a < nodes && meets(tr, a, mine);
            const bool hb = b >= 0 && b < nodes && meets(tr, b, mine);
            if (ha && hb) {
                if (sp < STACK) stack[BT * sp++] = b;
                node = a;
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
}

// lane i takes the face of leaf i; false for a lane past the faces and for an order[i] outside 0 .. F-1 (not a tree of build_nodes)
__device__ __forceinline__ bool lane_face(const Tree& tr, int& f) {
    const long long i = (long long)blockIdx.x * BT + threadIdx.x;
    if (i >= tr.nf) return false;
    const uint32_t fu = tr.order[i];
    f = (int)fu;
    return fu < (uint32_t)tr.nf;
}

__global__ void __launch_bounds__(BT) bvh_self_count_kernel(Tree tr, int32_t* __restrict__ n_all, int32_t* __restrict__ n_up) {
    __shared__ int stack[STACK * BT];
    int f;
    if (!lane_face(tr, f)) return;
    Tri mine;
    int all = 0, up = 0;
    if (load_tri(tr, f, mine)) self_walk<false>(tr, f, mine, stack + threadIdx.x, all, up, nullptr, 0, 0);
    n_all[f] = all;
    n_up[f] = up;
}

__global__ void __launch_bounds__(BT) bvh_self_emit_kernel(Tree tr, const int32_t* __restrict__ offsets, int num_pairs, int32_t* __restrict__ pairs) {
    __shared__ int stack[STACK * BT];
    int f;
    if (!lane_face(tr, f)) return;
    Tri mine;
    int all, up;
    const long long first = offsets[f], last = min((long long)offsets[f + 1], (long long)num_pairs);
    if (first >= 0 && first < last && load_tri(tr, f, mine)) self_walk<true>(tr, f, mine, stack + threadIdx.x, all, up, pairs, first, last);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The census.  A face is COUNTED when it is present and its three indices differ.
__device__ __forceinline__ bool counted(int i0, int i1, int i2) { return i0 != i1 && i1 != i2 && i2 != i0; }

// over v's list [start, end): the counted entries whose next neighbour is u, and those whose previous neighbour is u
__device__ __forceinline__ void directed(const Lists& L, int start, int end, int u, int& next_u, int& prev_u) {
    next_u = 0, prev_u = 0;
    for (int j = start; j < end; ++j) {
        int k, j0, j1, j2;
        if (!L.entry(j, k, j0, j1, j2) || !counted(j0, j1, j2)) continue;
        next_u += corner_at(k, 1, j0, j1, j2) == u ? 1 : 0;
        prev_u += corner_at(k, 2, j0, j1, j2) == u ? 1 : 0;
    }
}

// same and opposite of corner c = 3 f + k
__device__ __forceinline__ void edge_census_at(const Lists& L, long long c, int& ns, int& no) {
    const int k = (int)(c % 3);
    int i0, i1, i2;
    ns = -1, no = -1;
    if (load_face(L.faces, c / 3, L.nv, i0, i1, i2) && counted(i0, i1, i2)) {
        int start, end;
        L.range(corner_at(k, 0, i0, i1, i2), start, end);
        directed(L, start, end, corner_at(k, 1, i0, i1, i2), ns, no);
    }
}

__global__ void __launch_bounds__(NT) mesh_edge_census_kernel(Lists L, int32_t* __restrict__ same, int32_t* __restrict__ opposite) {
    const long long c = (long long)blockIdx.x * NT + threadIdx.x;
    if (c >= 3LL * L.nf) return;
    int ns, no;
    edge_census_at(L, c, ns, no);
    same[c] = ns;
    opposite[c] = no;
}

// the flag word of vertex v
__device__ __forceinline__ int vertex_census_at(const Lists& L, long long v) {
    int start, end;
    L.range(v, start, end);
    int bits = 0;
    for (int i = start; i < end; ++i) {
        int k, i0, i1, i2;
        if (!L.entry(i, k, i0, i1, i2) || !counted(i0, i1, i2)) continue;
        for (int s = 1; s <= 2; ++s) {
            int out, in;                                     // faces that run v -> u, and u -> v
            directed(L, start, end, corner_at(k, s, i0, i1, i2), out, in);
            bits |= out + in == 1 ? 1 : 0;
            bits |= out + in >= 3 ? 2 : 0;
            bits |= (out == 2 && in == 0) || (in == 2 && out == 0) ? 4 : 0;
        }
    }
    if (bits == 0) {
        const int n_v = L.count(start, end, end - start);
        if (n_v > 0 && !closed_fan(L, (int)v, start, end, n_v)) bits = 8;
    }
    return bits;
}

__global__ void __launch_bounds__(NT) mesh_vertex_census_kernel(Lists L, int32_t* __restrict__ flags) {
    const long long v = (long long)blockIdx.x * NT + threadIdx.x;
    if (v >= L.nv) return;
    flags[v] = vertex_census_at(L, v);
}

}  // namespace

extern "C" int v3d_recon_bvh_self_count(const int32_t* left, const int32_t* right, const uint32_t* order, const float* lo, const float* hi,
                                        const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, int32_t* n_all, int32_t* n_up,
                                        v3d_stream_t stream) {
    RECON_REQUIRE(n_all && n_up, "v3d_recon_bvh_self_count: null argument");
    BVH_REQUIRE_TREE("v3d_recon_bvh_self_count", left, right, order, lo, hi, verts, num_verts, faces, num_faces);
    const Tree tr{left, right, (const int32_t*)order, lo, hi, verts, faces, (int)num_verts, (int)num_faces};
    hipLaunchKernelGGL(bvh_self_count_kernel, dim3(nblk_bt(num_faces)), dim3(BT), 0, ST, tr, n_all, n_up);
    return check_launch("v3d_recon_bvh_self_count");
}

extern "C" int v3d_recon_bvh_self_emit(const int32_t* left, const int32_t* right, const uint32_t* order, const float* lo, const float* hi,
                                       const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* offsets,
                                       int32_t num_pairs, int32_t* pairs, v3d_stream_t stream) {
    RECON_REQUIRE(offsets && pairs, "v3d_recon_bvh_self_emit: null argument");
    BVH_REQUIRE_TREE("v3d_recon_bvh_self_emit", left, right, order, lo, hi, verts, num_verts, faces, num_faces);
    RECON_REQUIRE(num_pairs > 0, "v3d_recon_bvh_self_emit: num_pairs must be positive");
    const Tree tr{left, right, (const int32_t*)order, lo, hi, verts, faces, (int)num_verts, (int)num_faces};
    hipLaunchKernelGGL(bvh_self_emit_kernel, dim3(nblk_bt(num_faces)), dim3(BT), 0, ST, tr, offsets, (int)num_pairs, pairs);
    return check_launch("v3d_recon_bvh_self_emit");
}

extern "C" int v3d_recon_mesh_edge_census(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                                          int32_t* same, int32_t* opposite, v3d_stream_t stream) {
    RECON_REQUIRE(faces && ranges && corners && same && opposite, "v3d_recon_mesh_edge_census: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_mesh_edge_census", num_verts, num_faces);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(mesh_edge_census_kernel, dim3(nblk(3LL * num_faces)), dim3(NT), 0, ST, L, same, opposite);
    return check_launch("v3d_recon_mesh_edge_census");
}

extern "C" int v3d_recon_mesh_vertex_census(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                                            int32_t* flags, v3d_stream_t stream) {
    RECON_REQUIRE(faces && ranges && corners && flags, "v3d_recon_mesh_vertex_census: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_mesh_vertex_census", num_verts, num_faces);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(mesh_vertex_census_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, L, flags);
    return check_launch("v3d_recon_mesh_vertex_census");
}
