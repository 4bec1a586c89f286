// Repair what the mesh check reports (include/v3d_recon.h "Mesh repair", libv3d_recon.so; host side: v3d_amd/recon/mesh_repair.py): weld the
// vertices that coincide, drop the faces that are none, give every orientable patch one winding, cut out the faces in trouble and fan the
// open loops shut.  Every pass reads what the check already writes (same / opposite / flags of the census, per_face of the self-pair walk) and
// walks the vertex -> corner lists of mesh_lists.h (struct Lists, load_face); the area rule is no_area of bvh_walk.h.  The sorts and scans
// between the kernels are v3d_gs_radix_sort_pairs and v3d_gs_scan, called by the host.
//
// No atomics.  Every output element has one owner, except the flag words (changed, nonorient), where every writer stores the same 1.  All
// decisions are integer comparisons but two: equality of float32 coordinates by value (weld) and no_area (drop).  The only arithmetic is the
// float64 sum of a loop's vertices in ascending index, divided once and rounded once to float32; contraction is off, and there is no product
// to fuse anyway.  Two runs are bit-equal.
//
// Every kernel is a bounds check around one function of the element's index (weld_key_at, drop_bits_at, ..), so the same functions compile
// for the host and run there in a stand-alone program under the sanitizers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bvh_walk.h"
#include "mesh_lists.h"
#include "recon_host.h"
#include "v3d_recon.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ bool counted(int i0, int i1, int i2) { return i0 != i1 && i1 != i2 && i2 != i0; }

// the bits of x with -0.0 taken as +0.0: equal bits <=> equal value, for finite x
__device__ __forceinline__ uint32_t coord_bits(float x) { return x == 0.f ? 0u : __float_as_uint(x); }

// the face of corners[j], or -1 for a corner outside 0 .. 3F-1
__device__ __forceinline__ int face_of_entry(const Lists& L, int j) {
    const long long c = L.corners[j];
    return c < 0 || c >= 3LL * L.nf ? -1 : (int)(c / 3);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// 1. WELD
__device__ __forceinline__ void weld_key_at(const float* __restrict__ verts, long long v, unsigned long long& kz, unsigned long long& kxy) {
    kz = coord_bits(verts[3 * v + 2]);
    kxy = ((unsigned long long)coord_bits(verts[3 * v]) << 32) | coord_bits(verts[3 * v + 1]);
}

// does the i-th vertex of the sorted order differ from its predecessor (by value)?
__device__ __forceinline__ int weld_head_at(const float* __restrict__ verts, int nv, const int32_t* __restrict__ order, long long i) {
    if (i == 0) return 1;
    const int o = order[i], p = order[i - 1];
    if (!in_range(o, nv) || !in_range(p, nv)) return 1;
    const float* a = verts + 3 * (long long)o;
    const float* b = verts + 3 * (long long)p;
    return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] ? 0 : 1;
}

__global__ void __launch_bounds__(NT) weld_keys_kernel(const float* __restrict__ verts, int nv, unsigned long long* __restrict__ keys_z,
                                                       unsigned long long* __restrict__ keys_xy, uint32_t* __restrict__ vals) {
    const long long v = (long long)blockIdx.x * NT + threadIdx.x;
    if (v >= nv) return;
    unsigned long long kz, kxy;
    weld_key_at(verts, v, kz, kxy);
    keys_z[v] = kz;
    keys_xy[v] = kxy;
    vals[v] = (uint32_t)v;
}

__global__ void __launch_bounds__(NT) weld_heads_kernel(const float* __restrict__ verts, int nv, const int32_t* __restrict__ order,
                                                        int32_t* __restrict__ heads) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= nv) return;
    heads[i] = weld_head_at(verts, nv, order, i);
}

// first[g] = the vertex at the head of group g (offsets: the exclusive scan of heads)
__global__ void __launch_bounds__(NT) weld_first_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ heads,
                                                        const int32_t* __restrict__ offsets, int nv, int32_t* __restrict__ first) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= nv || heads[i] == 0) return;
    const int g = offsets[i];
    if (in_range(g, nv)) first[g] = order[i];
}

__device__ __forceinline__ int weld_remap_at(const int32_t* __restrict__ offsets, const int32_t* __restrict__ first, int nv, long long i, int o) {
    const int g = offsets[i + 1] - 1;                         // heads up to and including i, less one
    const int r = in_range(g, nv) ? first[g] : o;
    return in_range(r, nv) ? r : o;
}

__global__ void __launch_bounds__(NT) weld_remap_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ offsets,
                                                        const int32_t* __restrict__ first, int nv, int32_t* __restrict__ remap) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= nv) return;
    const int o = order[i];
    if (in_range(o, nv)) remap[o] = weld_remap_at(offsets, first, nv, i, o);
}

__global__ void __launch_bounds__(NT) remap_faces_kernel(const int32_t* __restrict__ faces, int nf, int nv, const int32_t* __restrict__ remap,
                                                         int32_t* __restrict__ faces_out) {
    const long long f = (long long)blockIdx.x * NT + threadIdx.x;
    if (f >= nf) return;
    int i0, i1, i2;
    if (load_face(faces, f, nv, i0, i1, i2)) {
        const int r0 = remap[i0], r1 = remap[i1], r2 = remap[i2];
        i0 = in_range(r0, nv) ? r0 : i0;
        i1 = in_range(r1, nv) ? r1 : i1;
        i2 = in_range(r2, nv) ? r2 : i2;
    }
    faces_out[3 * f] = i0;                                    // (an absent face is copied as it is)
    faces_out[3 * f + 1] = i1;
    faces_out[3 * f + 2] = i2;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// 2. DROP
__device__ __forceinline__ void sorted3(int i0, int i1, int i2, int& lo, int& mid, int& hi) {
    lo = min(i0, min(i1, i2));
    hi = max(i0, max(i1, i2));
    mid = (int)((long long)i0 + i1 + i2 - lo - hi);
}

__device__ __forceinline__ int drop_bits_at(const float* __restrict__ verts, const Lists& L, long long f) {
    int i0, i1, i2;
    if (!load_face(L.faces, f, L.nv, i0, i1, i2)) return 1;
    int bits = counted(i0, i1, i2) ? 0 : 2;
    const float* a = verts + 3 * (long long)i0;
    const float* b = verts + 3 * (long long)i1;
    const float* c = verts + 3 * (long long)i2;
    if (no_area(b[0] - a[0], b[1] - a[1], b[2] - a[2], c[0] - a[0], c[1] - a[1], c[2] - a[2])) bits |= 4;
    if (bits & 2) return bits;
    int lo, mid, hi, start, end;
    sorted3(i0, i1, i2, lo, mid, hi);
    L.range(lo, start, end);
    for (int j = start; j < end; ++j) {
        const int g = face_of_entry(L, j);
        int j0, j1, j2, glo, gmid, ghi;
        if (g < 0 || g >= f || !load_face(L.faces, g, L.nv, j0, j1, j2)) continue;
        sorted3(j0, j1, j2, glo, gmid, ghi);
        if (glo == lo && gmid == mid && ghi == hi) bits |= 8;
    }
    return bits;
}

__global__ void __launch_bounds__(NT) drop_flags_kernel(const float* __restrict__ verts, Lists L, int32_t* __restrict__ drop) {
    const long long f = (long long)blockIdx.x * NT + threadIdx.x;
    if (f >= L.nf) return;
    drop[f] = drop_bits_at(verts, L, f);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// 3. ORIENT.  The face across half-edge k of the counted face f = (i0, i1, i2), where the census says exactly two counted faces lie on that
// edge: the other counted entry of i_k's list that runs along i_k i_(k+1), the same way (rel = 1) or the other way (rel = 0).
__device__ __forceinline__ bool across(const Lists& L, const int32_t* __restrict__ same, const int32_t* __restrict__ opposite, long long f, int k, int i0,
                                       int i1, int i2, int& g, int& rel) {
    const int s = same[3 * f + k], o = opposite[3 * f + k];
    if (s < 1 || o < 0 || s + o != 2) return false;
    rel = s == 2 ? 1 : 0;
    const int u = corner_at(k, 0, i0, i1, i2), w = corner_at(k, 1, i0, i1, i2);
    int start, end;
    L.range(u, start, end);
    for (int j = start; j < end; ++j) {
        const int h = face_of_entry(L, j);
        int kk, j0, j1, j2;
        if (h < 0 || h == f || !L.entry(j, kk, j0, j1, j2) || !counted(j0, j1, j2)) continue;
        if (corner_at(kk, rel ? 1 : 2, j0, j1, j2) == w) {
            g = h;
            return true;
        }
    }
    return false;
}

__device__ __forceinline__ int orient_label_at(const Lists& L, const int32_t* __restrict__ same, const int32_t* __restrict__ opposite,
                                               const int32_t* __restrict__ lab, long long f) {
    int m = lab[f], i0, i1, i2;
    if (!load_face(L.faces, f, L.nv, i0, i1, i2) || !counted(i0, i1, i2)) return m;
    for (int k = 0; k < 3; ++k) {
        int g, rel;
        if (across(L, same, opposite, f, k, i0, i1, i2, g, rel)) m = min(m, lab[g] ^ rel);
    }
    return m;
}

// the root that f's patch must mark, or -1
__device__ __forceinline__ int orient_conflict_at(const Lists& L, const int32_t* __restrict__ same, const int32_t* __restrict__ opposite,
                                                  const int32_t* __restrict__ lab, long long f) {
    int i0, i1, i2;
    if (!load_face(L.faces, f, L.nv, i0, i1, i2) || !counted(i0, i1, i2)) return -1;
    const int mine = lab[f];
    for (int k = 0; k < 3; ++k) {
        int g, rel;
        if (!across(L, same, opposite, f, k, i0, i1, i2, g, rel)) continue;
        const int other = lab[g];
        if ((mine >> 1) == (other >> 1) && ((mine ^ other) & 1) != rel) return mine >> 1;
    }
    return -1;
}

__global__ void __launch_bounds__(NT) orient_round_kernel(Lists L, const int32_t* __restrict__ same, const int32_t* __restrict__ opposite,
                                                          const int32_t* __restrict__ lab_in, int32_t* __restrict__ lab_out, int32_t* __restrict__ changed) {
    const long long f = (long long)blockIdx.x * NT + threadIdx.x;
    if (f >= L.nf) return;
    const int out = orient_label_at(L, same, opposite, lab_in, f);
    lab_out[f] = out;
    if (out != lab_in[f]) *changed = 1;                       // (every writer stores the same value)
}

__global__ void __launch_bounds__(NT) orient_conflicts_kernel(Lists L, const int32_t* __restrict__ same, const int32_t* __restrict__ opposite,
                                                              const int32_t* __restrict__ lab, int32_t* __restrict__ nonorient) {
    const long long f = (long long)blockIdx.x * NT + threadIdx.x;
    if (f >= L.nf) return;
    const int root = orient_conflict_at(L, same, opposite, lab, f);
    if (in_range(root, L.nf)) nonorient[root] = 1;            // (every writer stores the same value)
}

__device__ __forceinline__ bool orient_swap_at(const int32_t* __restrict__ lab, const int32_t* __restrict__ nonorient, const int32_t* __restrict__ patch_flip,
                                               int nf, long long f) {
    const int l = lab[f], root = l >> 1;
    if (!in_range(root, nf) || nonorient[root] != 0) return false;
    return ((l & 1) ^ (patch_flip != nullptr && patch_flip[root] != 0 ? 1 : 0)) != 0;
}

__global__ void __launch_bounds__(NT) orient_apply_kernel(const int32_t* __restrict__ faces, int nf, const int32_t* __restrict__ lab,
                                                          const int32_t* __restrict__ nonorient, const int32_t* __restrict__ patch_flip,
                                                          int32_t* __restrict__ faces_out) {
    const long long f = (long long)blockIdx.x * NT + threadIdx.x;
    if (f >= nf) return;
    const bool swap = orient_swap_at(lab, nonorient, patch_flip, nf, f);
    const int i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    faces_out[3 * f] = faces[3 * f];
    faces_out[3 * f + 1] = swap ? i2 : i1;
    faces_out[3 * f + 2] = swap ? i1 : i2;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// 4. CUT
__device__ __forceinline__ void vertex_open_at(const Lists& L, const int32_t* __restrict__ same, const int32_t* __restrict__ opposite,
                                               const int32_t* __restrict__ flags, long long v, int& bad, int& next) {
    int start, end, n_out = 0;
    L.range(v, start, end);
    next = -1;
    for (int j = start; j < end; ++j) {
        const long long c = L.corners[j];
        if (c < 0 || c >= 3LL * L.nf || same[c] != 1 || opposite[c] != 0) continue;
        int a, b;
        if (!L.neighbours(j, a, b)) continue;
        if (n_out == 0) next = a;
        ++n_out;
    }
    if (n_out != 1) next = -1;
    bad = (flags[v] & (2 | 4 | 8)) != 0 || n_out >= 2 ? 1 : 0;
}

__global__ void __launch_bounds__(NT) vertex_open_kernel(Lists L, const int32_t* __restrict__ same, const int32_t* __restrict__ opposite,
                                                         const int32_t* __restrict__ flags, int32_t* __restrict__ bad, int32_t* __restrict__ next) {
    const long long v = (long long)blockIdx.x * NT + threadIdx.x;
    if (v >= L.nv) return;
    int b, n;
    vertex_open_at(L, same, opposite, flags, v, b, n);
    bad[v] = b;
    next[v] = n;
}

__global__ void __launch_bounds__(NT) trouble_kernel(const int32_t* __restrict__ faces, int nf, int nv, const int32_t* __restrict__ per_face,
                                                     const int32_t* __restrict__ bad, int32_t* __restrict__ trouble) {
    const long long f = (long long)blockIdx.x * NT + threadIdx.x;
    if (f >= nf) return;
    int i0, i1, i2, t = 0;
    if (load_face(faces, f, nv, i0, i1, i2)) t = per_face[f] > 0 || bad[i0] != 0 || bad[i1] != 0 || bad[i2] != 0 ? 1 : 0;
    trouble[f] = t;
}

__device__ __forceinline__ int grow_at(const Lists& L, const int32_t* __restrict__ in, long long f) {
    if (in[f] != 0) return 1;
    int i0, i1, i2;
    if (!load_face(L.faces, f, L.nv, i0, i1, i2)) return 0;
    for (int k = 0; k < 3; ++k) {
        int start, end;
        L.range(corner_at(k, 0, i0, i1, i2), start, end);
        for (int j = start; j < end; ++j) {
            const int g = face_of_entry(L, j);
            int a, b;
            if (g >= 0 && in[g] != 0 && L.neighbours(j, a, b)) return 1;
        }
    }
    return 0;
}

__global__ void __launch_bounds__(NT) grow_kernel(Lists L, const int32_t* __restrict__ in, int32_t* __restrict__ out) {
    const long long f = (long long)blockIdx.x * NT + threadIdx.x;
    if (f >= L.nf) return;
    out[f] = grow_at(L, in, f);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// 5. FILL
__global__ void __launch_bounds__(NT) loop_round_kernel(int nv, const int32_t* __restrict__ lab_in, const int32_t* __restrict__ jump_in,
                                                        int32_t* __restrict__ lab_out, int32_t* __restrict__ jump_out) {
    const long long v = (long long)blockIdx.x * NT + threadIdx.x;
    if (v >= nv) return;
    const int j = jump_in[v];
    const bool live = in_range(j, nv);
    lab_out[v] = live ? min(lab_in[v], lab_in[j]) : lab_in[v];
    jump_out[v] = live ? jump_in[j] : -1;
}

struct Loops {
    const int32_t* __restrict__ next;
    const int32_t* __restrict__ ranges;                       // [V][2]: label x's rows of members
    const int32_t* __restrict__ members;                      // [V]: the vertices sorted by label, ascending within one label
    int nv;
};

// 0: x heads no loop;  1: fillable;  2: a loop that is left.  n: its length
__device__ __forceinline__ int loop_state_at(const Loops& P, const int32_t* __restrict__ bad, const int32_t* __restrict__ label,
                                             const int32_t* __restrict__ jump, int max_hole_edges, long long x, int& n) {
    n = 0;
    if (!in_range(jump[x], P.nv) || label[x] != x) return 0;
    const int s = max(P.ranges[2 * x], 0), e = min(P.ranges[2 * x + 1], P.nv);
    n = max(e - s, 0);
    if (n < 3 || n > max_hole_edges) return 2;
    int u = P.next[x], steps = 1;
    while (steps < n && in_range(u, P.nv) && u != x && bad[u] == 0 && label[u] == x) {
        u = P.next[u];
        ++steps;
    }
    return u == x && steps == n ? 1 : 2;
}

__global__ void __launch_bounds__(NT) loop_flags_kernel(Loops P, const int32_t* __restrict__ bad, const int32_t* __restrict__ label,
                                                        const int32_t* __restrict__ jump, int max_hole_edges, int32_t* __restrict__ state,
                                                        int32_t* __restrict__ length) {
    const long long x = (long long)blockIdx.x * NT + threadIdx.x;
    if (x >= P.nv) return;
    int n;
    state[x] = loop_state_at(P, bad, label, jump, max_hole_edges, x, n);
    length[x] = n;
}

struct FillOut {
    const int32_t* __restrict__ face_off;
    const int32_t* __restrict__ vert_off;
    int n_faces, n_verts;
    int32_t* __restrict__ faces;
    float* __restrict__ verts;
    float* __restrict__ colors;
};

// the mean of n rows of `rows` [V][3], summed in float64 in the order of members[s ..], divided once, rounded once
__device__ __forceinline__ void mean_of(const float* __restrict__ rows, const Loops& P, int s, int n, float* __restrict__ out) {
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int j = 0; j < n; ++j) {
        const int u = P.members[s + j];
        if (!in_range(u, P.nv)) continue;
        sx += (double)rows[3 * (long long)u];
        sy += (double)rows[3 * (long long)u + 1];
        sz += (double)rows[3 * (long long)u + 2];
    }
    out[0] = (float)(sx / (double)n);
    out[1] = (float)(sy / (double)n);
    out[2] = (float)(sz / (double)n);
}

__device__ __forceinline__ void fill_loop_at(const float* __restrict__ verts, const float* __restrict__ colors, const Loops& P, const FillOut& O, long long x,
                                             int n) {
    const long long fo = O.face_off[x];
    const int s = P.ranges[2 * x];
    if (n < 3 || s < 0 || (long long)s + n > P.nv || fo < 0 || fo + (n == 3 ? 1 : n) > O.n_faces) return;
    if (n == 3) {
        const int n1 = P.next[x], n2 = in_range(n1, P.nv) ? P.next[n1] : -1;
        O.faces[3 * fo] = in_range(n2, P.nv) ? n2 : (int)x;
        O.faces[3 * fo + 1] = in_range(n1, P.nv) ? n1 : (int)x;
        O.faces[3 * fo + 2] = (int)x;
        return;
    }
    const int vo = O.vert_off[x];
    if (!in_range(vo, O.n_verts)) return;
    mean_of(verts, P, s, n, O.verts + 3 * (long long)vo);
    if (colors != nullptr) mean_of(colors, P, s, n, O.colors + 3 * (long long)vo);
    for (int j = 0; j < n; ++j) {
        const int u = P.members[s + j];
        const int w = in_range(u, P.nv) ? P.next[u] : -1;
        O.faces[3 * (fo + j)] = in_range(w, P.nv) ? w : u;
        O.faces[3 * (fo + j) + 1] = u;
        O.faces[3 * (fo + j) + 2] = P.nv + vo;
    }
}

__global__ void __launch_bounds__(NT) fill_emit_kernel(const float* __restrict__ verts, const float* __restrict__ colors, Loops P,
                                                       const int32_t* __restrict__ state, const int32_t* __restrict__ length, FillOut O) {
    const long long x = (long long)blockIdx.x * NT + threadIdx.x;
    if (x >= P.nv || state[x] != 1) return;
    fill_loop_at(verts, colors, P, O, x, length[x]);
}

inline bool verts_ok(int32_t nv) { return nv > 0; }

}  // namespace

#define REPAIR_REQUIRE_VERTS(name, nv) RECON_REQUIRE(verts_ok(nv), name ": num_verts %d must be positive", (int)(nv))

extern "C" int v3d_recon_repair_weld_keys(const float* verts, int32_t num_verts, uint64_t* keys_z, uint64_t* keys_xy, uint32_t* vals,
                                          v3d_stream_t stream) {
    RECON_REQUIRE(verts && keys_z && keys_xy && vals, "v3d_recon_repair_weld_keys: null argument");
    REPAIR_REQUIRE_VERTS("v3d_recon_repair_weld_keys", num_verts);
    hipLaunchKernelGGL(weld_keys_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, verts, (int)num_verts, (unsigned long long*)keys_z,
                       (unsigned long long*)keys_xy, vals);
    return check_launch("v3d_recon_repair_weld_keys");
}

extern "C" int v3d_recon_repair_weld_heads(const float* verts, int32_t num_verts, const int32_t* order, int32_t* heads, v3d_stream_t stream) {
    RECON_REQUIRE(verts && order && heads, "v3d_recon_repair_weld_heads: null argument");
    REPAIR_REQUIRE_VERTS("v3d_recon_repair_weld_heads", num_verts);
    hipLaunchKernelGGL(weld_heads_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, verts, (int)num_verts, order, heads);
    return check_launch("v3d_recon_repair_weld_heads");
}

extern "C" int v3d_recon_repair_weld_first(const int32_t* order, const int32_t* heads, const int32_t* offsets, int32_t num_verts, int32_t* first,
                                           v3d_stream_t stream) {
    RECON_REQUIRE(order && heads && offsets && first, "v3d_recon_repair_weld_first: null argument");
    REPAIR_REQUIRE_VERTS("v3d_recon_repair_weld_first", num_verts);
    hipLaunchKernelGGL(weld_first_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, order, heads, offsets, (int)num_verts, first);
    return check_launch("v3d_recon_repair_weld_first");
}

extern "C" int v3d_recon_repair_weld_remap(const int32_t* order, const int32_t* offsets, const int32_t* first, int32_t num_verts, int32_t* remap,
                                           v3d_stream_t stream) {
    RECON_REQUIRE(order && offsets && first && remap, "v3d_recon_repair_weld_remap: null argument");
    REPAIR_REQUIRE_VERTS("v3d_recon_repair_weld_remap", num_verts);
    hipLaunchKernelGGL(weld_remap_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, order, offsets, first, (int)num_verts, remap);
    return check_launch("v3d_recon_repair_weld_remap");
}

extern "C" int v3d_recon_repair_remap_faces(const int32_t* faces, int32_t num_faces, int32_t num_verts, const int32_t* remap, int32_t* faces_out,
                                            v3d_stream_t stream) {
    RECON_REQUIRE(faces && remap && faces_out, "v3d_recon_repair_remap_faces: null argument");
    RECON_REQUIRE(faces != faces_out, "v3d_recon_repair_remap_faces: faces and faces_out must be two buffers");
    MESH_REQUIRE_COUNTS("v3d_recon_repair_remap_faces", num_verts, num_faces);
    hipLaunchKernelGGL(remap_faces_kernel, dim3(nblk(num_faces)), dim3(NT), 0, ST, faces, (int)num_faces, (int)num_verts, remap, faces_out);
    return check_launch("v3d_recon_repair_remap_faces");
}

extern "C" int v3d_recon_repair_drop_flags(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                           const int32_t* corners, int32_t* drop, v3d_stream_t stream) {
    RECON_REQUIRE(verts && faces && ranges && corners && drop, "v3d_recon_repair_drop_flags: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_repair_drop_flags", num_verts, num_faces);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(drop_flags_kernel, dim3(nblk(num_faces)), dim3(NT), 0, ST, verts, L, drop);
    return check_launch("v3d_recon_repair_drop_flags");
}

extern "C" int v3d_recon_repair_orient_round(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                                             const int32_t* same, const int32_t* opposite, const int32_t* labels_in, int32_t* labels_out,
                                             int32_t* changed, v3d_stream_t stream) {
    RECON_REQUIRE(faces && ranges && corners && same && opposite && labels_in && labels_out && changed, "v3d_recon_repair_orient_round: null argument");
    RECON_REQUIRE(labels_in != labels_out, "v3d_recon_repair_orient_round: labels_in and labels_out must be two buffers");
    MESH_REQUIRE_COUNTS("v3d_recon_repair_orient_round", num_verts, num_faces);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(orient_round_kernel, dim3(nblk(num_faces)), dim3(NT), 0, ST, L, same, opposite, labels_in, labels_out, changed);
    return check_launch("v3d_recon_repair_orient_round");
}

extern "C" int v3d_recon_repair_orient_conflicts(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners,
                                                 int32_t num_verts, const int32_t* same, const int32_t* opposite, const int32_t* labels,
                                                 int32_t* nonorient, v3d_stream_t stream) {
    RECON_REQUIRE(faces && ranges && corners && same && opposite && labels && nonorient, "v3d_recon_repair_orient_conflicts: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_repair_orient_conflicts", num_verts, num_faces);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(orient_conflicts_kernel, dim3(nblk(num_faces)), dim3(NT), 0, ST, L, same, opposite, labels, nonorient);
    return check_launch("v3d_recon_repair_orient_conflicts");
}

extern "C" int v3d_recon_repair_orient_apply(const int32_t* faces, int32_t num_faces, const int32_t* labels, const int32_t* nonorient,
                                             const int32_t* patch_flip, int32_t* faces_out, v3d_stream_t stream) {
    RECON_REQUIRE(faces && labels && nonorient && faces_out, "v3d_recon_repair_orient_apply: null argument");
    RECON_REQUIRE(faces != faces_out, "v3d_recon_repair_orient_apply: faces and faces_out must be two buffers");
    RECON_REQUIRE(num_faces > 0, "v3d_recon_repair_orient_apply: num_faces %d must be positive", (int)num_faces);
    hipLaunchKernelGGL(orient_apply_kernel, dim3(nblk(num_faces)), dim3(NT), 0, ST, faces, (int)num_faces, labels, nonorient, patch_flip, faces_out);
    return check_launch("v3d_recon_repair_orient_apply");
}

extern "C" int v3d_recon_repair_vertex_open(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                                            const int32_t* same, const int32_t* opposite, const int32_t* flags, int32_t* bad, int32_t* next,
                                            v3d_stream_t stream) {
    RECON_REQUIRE(faces && ranges && corners && same && opposite && flags && bad && next, "v3d_recon_repair_vertex_open: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_repair_vertex_open", num_verts, num_faces);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(vertex_open_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, L, same, opposite, flags, bad, next);
    return check_launch("v3d_recon_repair_vertex_open");
}

extern "C" int v3d_recon_repair_trouble(const int32_t* faces, int32_t num_faces, int32_t num_verts, const int32_t* per_face, const int32_t* bad,
                                        int32_t* trouble, v3d_stream_t stream) {
    RECON_REQUIRE(faces && per_face && bad && trouble, "v3d_recon_repair_trouble: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_repair_trouble", num_verts, num_faces);
    hipLaunchKernelGGL(trouble_kernel, dim3(nblk(num_faces)), dim3(NT), 0, ST, faces, (int)num_faces, (int)num_verts, per_face, bad, trouble);
    return check_launch("v3d_recon_repair_trouble");
}

extern "C" int v3d_recon_repair_grow(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                                     const int32_t* trouble_in, int32_t* trouble_out, v3d_stream_t stream) {
    RECON_REQUIRE(faces && ranges && corners && trouble_in && trouble_out, "v3d_recon_repair_grow: null argument");
    RECON_REQUIRE(trouble_in != trouble_out, "v3d_recon_repair_grow: trouble_in and trouble_out must be two buffers");
    MESH_REQUIRE_COUNTS("v3d_recon_repair_grow", num_verts, num_faces);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(grow_kernel, dim3(nblk(num_faces)), dim3(NT), 0, ST, L, trouble_in, trouble_out);
    return check_launch("v3d_recon_repair_grow");
}

extern "C" int v3d_recon_repair_loop_round(int32_t num_verts, const int32_t* labels_in, const int32_t* jump_in, int32_t* labels_out, int32_t* jump_out,
                                           v3d_stream_t stream) {
    RECON_REQUIRE(labels_in && jump_in && labels_out && jump_out, "v3d_recon_repair_loop_round: null argument");
    RECON_REQUIRE(labels_in != labels_out && jump_in != jump_out, "v3d_recon_repair_loop_round: in and out must be two buffers");
    REPAIR_REQUIRE_VERTS("v3d_recon_repair_loop_round", num_verts);
    hipLaunchKernelGGL(loop_round_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, (int)num_verts, labels_in, jump_in, labels_out, jump_out);
    return check_launch("v3d_recon_repair_loop_round");
}

extern "C" int v3d_recon_repair_loop_flags(int32_t num_verts, const int32_t* next, const int32_t* bad, const int32_t* labels, const int32_t* jump,
                                           const int32_t* loop_ranges, const int32_t* members, int32_t max_hole_edges, int32_t* state, int32_t* length,
                                           v3d_stream_t stream) {
    RECON_REQUIRE(next && bad && labels && jump && loop_ranges && members && state && length, "v3d_recon_repair_loop_flags: null argument");
    REPAIR_REQUIRE_VERTS("v3d_recon_repair_loop_flags", num_verts);
    RECON_REQUIRE(max_hole_edges >= 3, "v3d_recon_repair_loop_flags: max_hole_edges %d must be at least 3", (int)max_hole_edges);
    const Loops P{next, loop_ranges, members, (int)num_verts};
    hipLaunchKernelGGL(loop_flags_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, P, bad, labels, jump, (int)max_hole_edges, state, length);
    return check_launch("v3d_recon_repair_loop_flags");
}

extern "C" int v3d_recon_repair_fill_emit(const float* verts, const float* colors, int32_t num_verts, const int32_t* next, const int32_t* loop_ranges,
                                          const int32_t* members, const int32_t* state, const int32_t* length, const int32_t* face_off,
                                          const int32_t* vert_off, int32_t num_new_faces, int32_t num_new_verts, int32_t* new_faces, float* new_verts,
                                          float* new_colors, v3d_stream_t stream) {
    RECON_REQUIRE(verts && next && loop_ranges && members && state && length && face_off && vert_off && new_faces,
                  "v3d_recon_repair_fill_emit: null argument");
    REPAIR_REQUIRE_VERTS("v3d_recon_repair_fill_emit", num_verts);
    RECON_REQUIRE(num_new_faces > 0 && num_new_verts >= 0 && (long long)num_verts + num_new_verts <= INT32_MAX,
                  "v3d_recon_repair_fill_emit: %d new faces must be positive, %d new vertices not negative, and %d + %d at most INT32_MAX", (int)num_new_faces,
                  (int)num_new_verts, (int)num_verts, (int)num_new_verts);
    RECON_REQUIRE(num_new_verts == 0 || (new_verts && (colors == nullptr || new_colors)), "v3d_recon_repair_fill_emit: null output for the new vertices");
    const Loops P{next, loop_ranges, members, (int)num_verts};
    const FillOut O{face_off, vert_off, (int)num_new_faces, (int)num_new_verts, new_faces, new_verts, new_colors};
    hipLaunchKernelGGL(fill_emit_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, verts, colors, P, state, length, O);
    return check_launch("v3d_recon_repair_fill_emit");
}
