// Decimation of the extracted mesh (include/v3d_recon.h "Mesh decimation", libv3d_recon.so; host side: v3d_amd/recon/mesh_decimate.py):
// quadric-error half-edge collapse v -> u in parallel rounds.  A round walks the vertex -> corner lists (mesh_lists.h: the walk, the
// closed-fan test and the integer rules of a collapse; the host rebuilds the lists from the live faces): every vertex proposes its cheapest
// valid collapse, two min-propagation launches accept the proposals whose key is the smallest within graph distance 2 (their stars are
// disjoint, their targets distinct), an optional cut keeps only as many as the target still allows, and the accepted collapses are applied
// per face.
//
// No atomics: every output element has one owner, which walks its lists in list order, and every launch reads what no thread of it writes
// (the one in-place update, Q_u += Q_v, has a single writer per u and reads rows that no accepted collapse writes).  Lists are short (a vertex
// above the valence cap proposes nothing and is no target), so a thread re-walks them instead of keeping them: no local arrays, no LDS.
// Positions are float32; every quadric, cost and normal test is computed in fp64 from them, without contraction, statement for statement as
// tests/mesh_decimate_ref.py writes them.  A dead face holds num_verts in all three places: like any face with an index outside 0 .. V-1 it
// is absent everywhere.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mesh_lists.h"
#include "recon_host.h"
#include "v3d_recon.h"

#pragma clang fp contract(off)

namespace {

// (p1 - p0) x (p2 - p0)
__device__ __forceinline__ D3 face_cross(const D3& p0, const D3& p1, const D3& p2) {
    const double ux = p1.x - p0.x, uy = p1.y - p0.y, uz = p1.z - p0.z;
    const double wx = p2.x - p0.x, wy = p2.y - p0.y, wz = p2.z - p0.z;
    return D3{uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx};
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Q_v: the sum in list order of area x (a b c d)^T (a b c d) over the planes a x + b y + c z + d = 0 of the incident faces, upper triangle
__global__ void __launch_bounds__(NT) mesh_vertex_quadrics_kernel(const float* __restrict__ verts, Lists L, double* __restrict__ quadrics) {
    const long long v = (long long)blockIdx.x * NT + threadIdx.x;
    if (v >= L.nv) return;
    int start, end;
    L.range(v, start, end);
    double q[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};          // (indexed by constants only, after unrolling: registers)
    for (int i = start; i < end; ++i) {
        int k, i0, i1, i2;
        if (!L.entry(i, k, i0, i1, i2)) continue;
        const D3 p0 = load_pos(verts, i0);
        const D3 n = face_cross(p0, load_pos(verts, i1), load_pos(verts, i2));
        const double len2 = n.x * n.x + n.y * n.y + n.z * n.z;
        if (!(len2 > 0.0)) continue;                          // a face without area has no plane
        const double len = sqrt(len2);
        const double a = n.x / len, b = n.y / len, c = n.z / len;
        const double d = -(a * p0.x + b * p0.y + c * p0.z);
        const double w = 0.5 * len;
        q[0] += w * (a * a);
        q[1] += w * (a * b);
        q[2] += w * (a * c);
        q[3] += w * (a * d);
        q[4] += w * (b * b);
        q[5] += w * (b * c);
        q[6] += w * (b * d);
        q[7] += w * (c * c);
        q[8] += w * (c * d);
        q[9] += w * (d * d);
    }
#pragma unroll
    for (int j = 0; j < 10; ++j) quadrics[10 * v + j] = q[j];
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The geometric half of a collapse's validity (the integer half is mesh_lists.h's collapse_topology_ok): does v -> u keep the side of every
// face of v's star [start, end) that survives it?
__device__ bool collapse_keeps_normals(const float* __restrict__ verts, const Lists& L, int start, int end, int u) {
    const D3 pu = load_pos(verts, u);
    for (int j = start; j < end; ++j) {                       // the faces that survive: v's faces without u
        int k, i0, i1, i2;
        if (!L.entry(j, k, i0, i1, i2)) continue;
        const int a = corner_at(k, 1, i0, i1, i2), b = corner_at(k, 2, i0, i1, i2);
        if (a == u || b == u) continue;
        const D3 p0 = load_pos(verts, i0), p1 = load_pos(verts, i1), p2 = load_pos(verts, i2);
        const D3 before = face_cross(p0, p1, p2);
        const D3 after = face_cross(k == 0 ? pu : p0, k == 1 ? pu : p1, k == 2 ? pu : p2);
        const double dot = before.x * after.x + before.y * after.y + before.z * after.z;
        if (!(dot > 0.0)) return false;                       // flipped, or without area before or after
    }
    return true;
}

__global__ void __launch_bounds__(NT) mesh_decim_propose_kernel(const float* __restrict__ verts, Lists L, const double* __restrict__ quadrics,
                                                                int max_valence, unsigned long long* __restrict__ keys, int32_t* __restrict__ targets) {
    const long long vv = (long long)blockIdx.x * NT + threadIdx.x;
    if (vv >= L.nv) return;
    const int v = (int)vv;
    unsigned long long key = NO_KEY;
    int target = -1;
    int start, end;
    L.range(v, start, end);
    const int n_v = L.count(start, end, max_valence);
    if (n_v >= 3 && n_v <= max_valence && closed_fan(L, v, start, end, n_v)) {
        unsigned best_bits = 0xffffffffu;
        for (int i = start; i < end; ++i) {
            int u, b;
            if (!L.neighbours(i, u, b)) continue;
            // (a conjunction of two pure tests.  The normal test goes first: it reads v's star alone, the integer half walks u's list once for
            // every neighbour of v, and a thread's time is its chain of dependent loads - 620 us against 800 us the other way round on a
            // 1344-face mesh)
            if (!(collapse_keeps_normals(verts, L, start, end, u) && collapse_topology_ok(L, v, start, end, n_v, u, i, max_valence))) continue;
            const D3 p = load_pos(verts, u);
            double q[10];
#pragma unroll
            for (int j = 0; j < 10; ++j) q[j] = quadrics[10 * vv + j] + quadrics[10 * (long long)u + j];
            double cost = p.x * (q[0] * p.x + q[1] * p.y + q[2] * p.z + q[3]) + p.y * (q[1] * p.x + q[4] * p.y + q[5] * p.z + q[6]) +
                          p.z * (q[2] * p.x + q[5] * p.y + q[7] * p.z + q[8]) + (q[3] * p.x + q[6] * p.y + q[8] * p.z + q[9]);
            if (!(cost == cost)) continue;                    // positions that are not finite: no proposal
            if (cost < 0.0) cost = 0.0;
            const unsigned bits = __float_as_uint((float)cost);
            if (bits == 0xffffffffu) continue;
            if (target < 0 || bits < best_bits || (bits == best_bits && u < target)) {
                best_bits = bits;
                target = u;
            }
        }
        if (target >= 0) key = ((unsigned long long)best_bits << 32) | (unsigned long long)(unsigned)v;
    }
    keys[vv] = key;
    targets[vv] = target;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// keys_out[v] = the smallest of keys_in over v and its neighbours
__global__ void __launch_bounds__(NT) mesh_decim_min_round_kernel(Lists L, const unsigned long long* __restrict__ keys_in,
                                                                  unsigned long long* __restrict__ keys_out) {
    const long long v = (long long)blockIdx.x * NT + threadIdx.x;
    if (v >= L.nv) return;
    int start, end;
    L.range(v, start, end);
    unsigned long long m = keys_in[v];
    for (int i = start; i < end; ++i) {
        int k, i0, i1, i2;
        if (!L.entry(i, k, i0, i1, i2)) continue;
        m = min(m, min(keys_in[i0], min(keys_in[i1], keys_in[i2])));
    }
    keys_out[v] = m;
}

__global__ void __launch_bounds__(NT) mesh_decim_accept_kernel(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ min2,
                                                               int nv, unsigned max_bits, int32_t* __restrict__ accept,
                                                               unsigned long long* __restrict__ sel_keys, uint32_t* __restrict__ sel_vals,
                                                               int32_t* __restrict__ flags) {
    const long long v = (long long)blockIdx.x * NT + threadIdx.x;
    if (v >= nv) return;
    const unsigned long long k = keys[v];
    const bool smallest = k != NO_KEY && min2[v] == k;
    const bool ok = smallest && (unsigned)(k >> 32) <= max_bits;
    accept[v] = ok ? 1 : 0;
    sel_keys[v] = ok ? k : NO_KEY;
    sel_vals[v] = (uint32_t)v;
    if (smallest) flags[0] = 1;                               // (every writer stores the same value)
    if (ok) flags[1] = 1;
}

// Row i of the sorted accepted keys keeps its vertex only while i < ceil((live - target) / 2)
__global__ void __launch_bounds__(NT) mesh_decim_cut_kernel(const unsigned long long* __restrict__ sel_keys_sorted, const uint32_t* __restrict__ sel_vals_sorted,
                                                            int nv, const int32_t* __restrict__ live_faces, int target, int32_t* __restrict__ accept) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= nv || sel_keys_sorted[i] == NO_KEY) return;
    const long long over = (long long)live_faces[0] - target;
    const long long quota = over > 0 ? (over + 1) / 2 : 0;
    const uint32_t v = sel_vals_sorted[i];
    if (i >= quota && v < (uint32_t)nv) accept[v] = 0;
}

// Thread t decides face t (t < nf) and vertex t (t < nv)
__global__ void __launch_bounds__(NT) mesh_decim_apply_kernel(const int32_t* __restrict__ faces_in, int nf, int nv, const int32_t* __restrict__ accept,
                                                              const int32_t* __restrict__ targets, int32_t* __restrict__ faces_out,
                                                              int32_t* __restrict__ live, double* __restrict__ quadrics, int32_t* __restrict__ removed) {
    const long long t = (long long)blockIdx.x * NT + threadIdx.x;
    if (t < nf) {
        int i0, i1, i2, alive = 0;
        if (load_face(faces_in, t, nv, i0, i1, i2)) {
            alive = 1;
            const int k = accept[i0] != 0 ? 0 : (accept[i1] != 0 ? 1 : (accept[i2] != 0 ? 2 : -1));          // (at most one corner is accepted)
            if (k >= 0) {
                const int u = targets[corner_at(k, 0, i0, i1, i2)];
                if (in_range(u, nv)) {
                    if (u == corner_at(k, 1, i0, i1, i2) || u == corner_at(k, 2, i0, i1, i2)) alive = 0;      // a face on the collapsed edge
                    else if (k == 0) i0 = u;
                    else if (k == 1) i1 = u;
                    else i2 = u;
                }
            }
        }
        faces_out[3 * t] = alive ? i0 : nv;
        faces_out[3 * t + 1] = alive ? i1 : nv;
        faces_out[3 * t + 2] = alive ? i2 : nv;
        live[t] = alive;
    }
    if (t < nv && accept[t] != 0) {
        const int u = targets[t];
        if (in_range(u, nv) && u != t) {
            // no accepted vertex is a target and no two share one: row u has this one writer, row t none
#pragma unroll
            for (int j = 0; j < 10; ++j) quadrics[10 * (long long)u + j] += quadrics[10 * t + j];
            removed[t] = 1;
        }
    }
}

}  // namespace

extern "C" int v3d_recon_mesh_vertex_quadrics(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                              const int32_t* corners, double* quadrics, v3d_stream_t stream) {
    RECON_REQUIRE(verts && faces && ranges && corners && quadrics, "v3d_recon_mesh_vertex_quadrics: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_mesh_vertex_quadrics", num_verts, num_faces);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(mesh_vertex_quadrics_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, verts, L, quadrics);
    return check_launch("v3d_recon_mesh_vertex_quadrics");
}

extern "C" int v3d_recon_mesh_decim_propose(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                            const int32_t* corners, const double* quadrics, int32_t max_valence, uint64_t* keys, int32_t* targets,
                                            v3d_stream_t stream) {
    RECON_REQUIRE(verts && faces && ranges && corners && quadrics && keys && targets, "v3d_recon_mesh_decim_propose: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_mesh_decim_propose", num_verts, num_faces);
    MESH_REQUIRE_VALENCE("v3d_recon_mesh_decim_propose", max_valence);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(mesh_decim_propose_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, verts, L, quadrics, (int)max_valence,
                       (unsigned long long*)keys, targets);
    return check_launch("v3d_recon_mesh_decim_propose");
}

extern "C" int v3d_recon_mesh_decim_min_round(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                                              const uint64_t* keys_in, uint64_t* keys_out, v3d_stream_t stream) {
    RECON_REQUIRE(faces && ranges && corners && keys_in && keys_out, "v3d_recon_mesh_decim_min_round: null argument");
    RECON_REQUIRE(keys_in != keys_out, "v3d_recon_mesh_decim_min_round: keys_in and keys_out must be two buffers");
    MESH_REQUIRE_COUNTS("v3d_recon_mesh_decim_min_round", num_verts, num_faces);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(mesh_decim_min_round_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, L, (const unsigned long long*)keys_in,
                       (unsigned long long*)keys_out);
    return check_launch("v3d_recon_mesh_decim_min_round");
}

extern "C" int v3d_recon_mesh_decim_accept(const uint64_t* keys, const uint64_t* min2, int32_t num_verts, float max_error, int32_t* accept,
                                           uint64_t* sel_keys, uint32_t* sel_vals, int32_t* flags, v3d_stream_t stream) {
    RECON_REQUIRE(keys && min2 && accept && sel_keys && sel_vals && flags, "v3d_recon_mesh_decim_accept: null argument");
    RECON_REQUIRE(num_verts > 0, "v3d_recon_mesh_decim_accept: num_verts %d must be positive", (int)num_verts);
    RECON_REQUIRE(max_error >= 0.f, "v3d_recon_mesh_decim_accept: max_error %g must be a number that is not negative", (double)max_error);
    union {
        float f;
        uint32_t u;
    } bits;
    bits.f = max_error + 0.f;                                 // (-0 -> +0: the costs are clamped at +0)
    hipLaunchKernelGGL(mesh_decim_accept_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, (const unsigned long long*)keys, (const unsigned long long*)min2,
                       (int)num_verts, (unsigned)bits.u, accept, (unsigned long long*)sel_keys, sel_vals, flags);
    return check_launch("v3d_recon_mesh_decim_accept");
}

extern "C" int v3d_recon_mesh_decim_cut(const uint64_t* sel_keys_sorted, const uint32_t* sel_vals_sorted, int32_t num_verts, const int32_t* live_faces,
                                        int32_t target_faces, int32_t* accept, v3d_stream_t stream) {
    RECON_REQUIRE(sel_keys_sorted && sel_vals_sorted && live_faces && accept, "v3d_recon_mesh_decim_cut: null argument");
    RECON_REQUIRE(num_verts > 0, "v3d_recon_mesh_decim_cut: num_verts %d must be positive", (int)num_verts);
    RECON_REQUIRE(target_faces >= 0, "v3d_recon_mesh_decim_cut: target_faces %d must not be negative", (int)target_faces);
    hipLaunchKernelGGL(mesh_decim_cut_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, (const unsigned long long*)sel_keys_sorted, sel_vals_sorted,
                       (int)num_verts, live_faces, (int)target_faces, accept);
    return check_launch("v3d_recon_mesh_decim_cut");
}

extern "C" int v3d_recon_mesh_decim_apply(const int32_t* faces_in, int32_t num_faces, int32_t num_verts, const int32_t* accept, const int32_t* targets,
                                          int32_t* faces_out, int32_t* live, double* quadrics, int32_t* removed, v3d_stream_t stream) {
    RECON_REQUIRE(faces_in && accept && targets && faces_out && live && quadrics && removed, "v3d_recon_mesh_decim_apply: null argument");
    RECON_REQUIRE(faces_in != faces_out, "v3d_recon_mesh_decim_apply: faces_in and faces_out must be two buffers");
    MESH_REQUIRE_COUNTS("v3d_recon_mesh_decim_apply", num_verts, num_faces);
    const long long n = num_faces > num_verts ? num_faces : num_verts;
    hipLaunchKernelGGL(mesh_decim_apply_kernel, dim3(nblk(n)), dim3(NT), 0, ST, faces_in, (int)num_faces, (int)num_verts, accept, targets, faces_out, live,
                       quadrics, removed);
    return check_launch("v3d_recon_mesh_decim_apply");
}
