// Isotropic remeshing of the mesh (include/v3d_recon.h "Mesh remeshing", libv3d_recon.so; host side: v3d_amd/recon/mesh_remesh.py): edge
// split, half-edge collapse and edge flip towards a target edge length L (Botsch & Kobbelt 2004: split above 4/3 L, collapse below 4/5 L,
// flip towards valence 6), tangential relaxation and reprojection onto the input mesh.  Every topological operation is proposed by a vertex
// on its own corner list (mesh_lists.h, rebuilt per round from the live faces by the host) as a 64-bit key; the selection is meshdecim.hip's
// (min_round twice, accept), which leaves accepted vertices at least 3 edges apart; the apply kernels, one thread per vertex, then write only
// faces that hold the accepted vertex itself, in place.
//
// No atomics: every output element has one owner.  Lists are short (a vertex above the valence cap proposes nothing), so a thread re-walks
// them instead of keeping them: no local arrays, no LDS.  Positions are float32; lengths are float32, (dx dx + dy dy) + dz dz, the normal
// tests are fp64, without contraction, statement for statement as tests/mesh_remesh_ref.py writes them.  A dead or unborn face holds
// num_verts in all three places: like any face with an index outside 0 .. V-1 it is absent everywhere.  The closed-fan walk and the integer
// rules of the collapse are meshdecim.hip's own: both call closed_fan and collapse_topology_ok of mesh_lists.h.
//
// The library is built with -ffast-math ... -fno-fast-math, which leaves -ffp-contract=fast behind: the pragma below states the intent but the
// compiler does not honour it, and a product that feeds a sum would be fused into an fma.  Every such product therefore goes through mul(),
// whose empty asm statement hides it from the contraction: the keys are compared bit for bit with a restatement that rounds every product.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mesh_lists.h"
#include "recon_host.h"
#include "v3d_recon.h"

#pragma clang fp contract(off)

namespace {

constexpr unsigned KEY_HASH = 0x9E3779B1u;                    // odd: v -> v * KEY_HASH mod 2^32 is a bijection, so keys stay distinct

__device__ __forceinline__ unsigned long long make_key(unsigned bits, int v) {
    return ((unsigned long long)bits << 32) | (unsigned long long)((unsigned)v * KEY_HASH);
}

// a b, rounded on its own: the empty asm keeps the product out of any fused multiply-add
__device__ __forceinline__ float mul(float a, float b) {
    float p = a * b;
    asm("" : "+v"(p));
    return p;
}
__device__ __forceinline__ double mul(double a, double b) {
    double p = a * b;
    asm("" : "+v"(p));
    return p;
}

// (p1 - p0) x (p2 - p0)
__device__ __forceinline__ D3 face_cross(const D3& p0, const D3& p1, const D3& p2) {
    const double ux = p1.x - p0.x, uy = p1.y - p0.y, uz = p1.z - p0.z;
    const double wx = p2.x - p0.x, wy = p2.y - p0.y, wz = p2.z - p0.z;
    return D3{mul(uy, wz) - mul(uz, wy), mul(uz, wx) - mul(ux, wz), mul(ux, wy) - mul(uy, wx)};
}

__device__ __forceinline__ double dot(const D3& a, const D3& b) { return mul(a.x, b.x) + mul(a.y, b.y) + mul(a.z, b.z); }

// |p_i - p_j|^2 in float: (dx dx + dy dy) + dz dz
__device__ __forceinline__ float dist2(const float* __restrict__ verts, long long i, long long j) {
    const float dx = verts[3 * i] - verts[3 * j], dy = verts[3 * i + 1] - verts[3 * j + 1], dz = verts[3 * i + 2] - verts[3 * j + 2];
    return (mul(dx, dx) + mul(dy, dy)) + mul(dz, dz);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Split: a proposes its longest editable edge above hi^2
__global__ void __launch_bounds__(NT) remesh_split_propose_kernel(const float* __restrict__ verts, Lists L, float L2, float hi2, int max_valence,
                                                                  unsigned long long* __restrict__ keys, int32_t* __restrict__ targets) {
    const long long aa = (long long)blockIdx.x * NT + threadIdx.x;
    if (aa >= L.nv) return;
    const int a = (int)aa;
    int start, end;
    L.range(a, start, end);
    const int n_a = L.count(start, end, max_valence);
    int target = -1;
    float best = 0.f;
    if (n_a >= 1 && n_a <= max_valence) {
        for (int i = start; i < end; ++i) {
            int b, y;
            if (!L.neighbours(i, b, y) || b == a) continue;
            const float len2 = dist2(verts, a, b);
            if (!(len2 > hi2)) continue;
            int ic, c, id, d;
            if (!L.editable(a, start, end, b, ic, c, id, d)) continue;
            if (target < 0 || len2 > best || (len2 == best && b < target)) {
                best = len2;
                target = b;
            }
        }
    }
    keys[aa] = target >= 0 ? make_key(__float_as_uint(L2 / best), a) : NO_KEY;
    targets[aa] = target;
}

// Thread a, accepted, of exclusive rank r: the new vertex V_live + r, the new faces F_live + 2 r and F_live + 2 r + 1.  Thread 0 writes the
// new counts.  Everything is read before the first store.
__global__ void __launch_bounds__(NT) remesh_split_apply_kernel(float* __restrict__ verts, float* __restrict__ colors, int32_t* faces, Lists L,
                                                                const int32_t* __restrict__ accept, const int32_t* __restrict__ targets,
                                                                const int32_t* __restrict__ rank, const int32_t* __restrict__ counts_in,
                                                                int32_t* __restrict__ counts_out, int32_t* __restrict__ flag) {
    const long long aa = (long long)blockIdx.x * NT + threadIdx.x;
    if (aa >= L.nv) return;
    const int vl = min(max(counts_in[0], 0), L.nv), fl = min(max(counts_in[1], 0), L.nf);
    const int total = max(rank[L.nv], 0);
    const int done = min(total, min(L.nv - vl, (L.nf - fl) / 2));
    if (aa == 0) {
        counts_out[0] = vl + done;
        counts_out[1] = fl + 2 * done;
        if (total > done) flag[0] = 1;
    }
    if (accept[aa] == 0) return;
    const int a = (int)aa, r = rank[aa], b = targets[aa];
    if (r < 0 || r >= done || !in_range(b, L.nv)) return;     // dropped by rank: nothing is written past a buffer
    int start, end, ic, c, id, d;
    L.range(a, start, end);
    if (!L.editable(a, start, end, b, ic, c, id, d)) return;
    const long long cc = L.corners[ic], cd = L.corners[id];
    const long long fc = cc / 3, fd = cd / 3;
    const int kc = (int)(cc % 3), kd = (int)(cd % 3);
    const long long m = (long long)vl + r, f0 = (long long)fl + 2LL * r, f1 = f0 + 1;
    const float mx = 0.5f * (verts[3 * aa] + verts[3 * (long long)b]), my = 0.5f * (verts[3 * aa + 1] + verts[3 * (long long)b + 1]),
                mz = 0.5f * (verts[3 * aa + 2] + verts[3 * (long long)b + 2]);
    const float cx = 0.5f * (colors[3 * aa] + colors[3 * (long long)b]), cy = 0.5f * (colors[3 * aa + 1] + colors[3 * (long long)b + 1]),
                cz = 0.5f * (colors[3 * aa + 2] + colors[3 * (long long)b + 2]);
    verts[3 * m] = mx;
    verts[3 * m + 1] = my;
    verts[3 * m + 2] = mz;
    colors[3 * m] = cx;
    colors[3 * m + 1] = cy;
    colors[3 * m + 2] = cz;
    faces[3 * fc + (kc + 1) % 3] = (int)m;                    // (a, b, c) -> (a, m, c)
    faces[3 * f0] = (int)m;                                   // + (m, b, c)
    faces[3 * f0 + 1] = b;
    faces[3 * f0 + 2] = c;
    faces[3 * fd + kd] = (int)m;                              // (b, a, d) -> (b, m, d)
    faces[3 * f1] = (int)m;                                   // + (m, a, d)
    faces[3 * f1 + 1] = a;
    faces[3 * f1 + 2] = d;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Collapse v -> u.  The geometric half of its validity (the integer half is mesh_lists.h's collapse_topology_ok), over v's star [start, end):
// no edge (u, w) may come out longer than hi, and every face that survives keeps its side.
__device__ bool collapse_keeps_shape(const float* __restrict__ verts, const Lists& L, int start, int end, int u, float hi2) {
    for (int j = start; j < end; ++j) {
        int w, b;
        if (L.neighbours(j, w, b) && w != u && dist2(verts, u, w) > hi2) return false;
    }
    const D3 pu = load_pos(verts, u);
    for (int j = start; j < end; ++j) {                       // the faces that survive: v's faces without u
        int k, i0, i1, i2;
        if (!L.entry(j, k, i0, i1, i2)) continue;
        const int a = corner_at(k, 1, i0, i1, i2), b = corner_at(k, 2, i0, i1, i2);
        if (a == u || b == u) continue;
        const D3 p0 = load_pos(verts, i0), p1 = load_pos(verts, i1), p2 = load_pos(verts, i2);
        const D3 before = face_cross(p0, p1, p2);
        const D3 after = face_cross(k == 0 ? pu : p0, k == 1 ? pu : p1, k == 2 ? pu : p2);
        if (!(dot(before, after) > 0.0)) return false;        // flipped, or without area before or after
    }
    return true;
}

__global__ void __launch_bounds__(NT) remesh_collapse_propose_kernel(const float* __restrict__ verts, Lists L, float lo2, float hi2, int max_valence,
                                                                     unsigned long long* __restrict__ keys, int32_t* __restrict__ targets) {
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
            const float len2 = dist2(verts, v, u);
            if (!(len2 < lo2)) continue;
            // (the geometric half first, as in meshdecim.hip and for its reason: the length cap turns most candidates down after a few loads)
            if (!(collapse_keeps_shape(verts, L, start, end, u, hi2) && collapse_topology_ok(L, v, start, end, n_v, u, i, max_valence))) continue;
            const unsigned bits = __float_as_uint(len2);
            if (target < 0 || bits < best_bits || (bits == best_bits && u < target)) {
                best_bits = bits;
                target = u;
            }
        }
        if (target >= 0) key = make_key(best_bits, v);
    }
    keys[vv] = key;
    targets[vv] = target;
}

// Thread v, accepted: every face of v's list dies when it holds targets[v], else names it in v's place.  The list is read through `corners`
// alone while the faces change: every face is read once, by the iteration that writes it.
__global__ void __launch_bounds__(NT) remesh_collapse_apply_kernel(int32_t* faces, Lists L, const int32_t* __restrict__ accept,
                                                                   const int32_t* __restrict__ targets, int32_t* __restrict__ removed) {
    const long long vv = (long long)blockIdx.x * NT + threadIdx.x;
    if (vv >= L.nv || accept[vv] == 0) return;
    const int v = (int)vv, u = targets[vv];
    if (!in_range(u, L.nv) || u == v) return;
    int start, end;
    L.range(v, start, end);
    for (int i = start; i < end; ++i) {
        int k, i0, i1, i2;
        if (!L.entry(i, k, i0, i1, i2)) continue;
        if (corner_at(k, 0, i0, i1, i2) != v) continue;       // (a stale entry: nothing to do with v)
        const long long f = L.corners[i] / 3;
        if (corner_at(k, 1, i0, i1, i2) == u || corner_at(k, 2, i0, i1, i2) == u) {
            faces[3 * f] = L.nv;
            faces[3 * f + 1] = L.nv;
            faces[3 * f + 2] = L.nv;
        } else {
            faces[3 * f + k] = u;
        }
    }
    removed[vv] = 1;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Flip: a proposes the editable edge (a, b) -> (c, d) that lowers the summed deviation from the target valences the most
__device__ __forceinline__ int deviation(int val, int target) { return val > target ? val - target : target - val; }

__global__ void __launch_bounds__(NT) remesh_flip_propose_kernel(const float* __restrict__ verts, Lists L, const int32_t* __restrict__ boundary,
                                                                 int max_valence, unsigned long long* __restrict__ keys, int32_t* __restrict__ targets) {
    const long long aa = (long long)blockIdx.x * NT + threadIdx.x;
    if (aa >= L.nv) return;
    const int a = (int)aa;
    int start, end;
    L.range(a, start, end);
    const int va = L.count(start, end, max_valence);
    int target = -1, best = 0;
    if (va > 3 && va <= max_valence) {
        const int ta = boundary[a] != 0 ? 4 : 6;
        for (int i = start; i < end; ++i) {
            int b, y;
            if (!L.neighbours(i, b, y)) continue;
            int ic, c, id, d;
            if (!L.editable(a, start, end, b, ic, c, id, d)) continue;
            const int vb = L.valence(b, max_valence);
            if (!(vb > 3 && vb <= max_valence)) continue;
            const int vc = L.valence(c, max_valence), vd = L.valence(d, max_valence);
            if (!(vc < max_valence && vd < max_valence)) continue;
            const int tb = boundary[b] != 0 ? 4 : 6, tc = boundary[c] != 0 ? 4 : 6, td = boundary[d] != 0 ? 4 : 6;
            const int gain = (deviation(va, ta) + deviation(vb, tb) + deviation(vc, tc) + deviation(vd, td)) -
                             (deviation(va - 1, ta) + deviation(vb - 1, tb) + deviation(vc + 1, tc) + deviation(vd + 1, td));
            if (gain <= 0) continue;
            if (!(target < 0 || gain > best || (gain == best && b < target))) continue;
            bool shared = false;                              // c and d already share a face: the flip would double the edge (c, d)
            int cs, ce;
            L.range(c, cs, ce);
            for (int m = cs; m < ce && !shared; ++m) {
                int x, z;
                shared = L.neighbours(m, x, z) && (x == d || z == d);
            }
            if (shared) continue;
            const D3 pa = load_pos(verts, a), pb = load_pos(verts, b), pc = load_pos(verts, c), pd = load_pos(verts, d);
            const D3 n1 = face_cross(pa, pb, pc), n2 = face_cross(pb, pa, pd);
            const D3 m1 = face_cross(pa, pd, pc), m2 = face_cross(pd, pb, pc);
            if (!(dot(m1, n1) > 0.0 && dot(m1, n2) > 0.0 && dot(m2, n1) > 0.0 && dot(m2, n2) > 0.0)) continue;
            best = gain;
            target = b;
        }
    }
    keys[aa] = target >= 0 ? make_key(__float_as_uint((float)(8 - best)), a) : NO_KEY;
    targets[aa] = target;
}

// Thread a, accepted: (a, b, c) -> (a, d, c) and (b, a, d) -> (d, b, c), both of a's own list, both read before the first store
__global__ void __launch_bounds__(NT) remesh_flip_apply_kernel(int32_t* faces, Lists L, const int32_t* __restrict__ accept,
                                                               const int32_t* __restrict__ targets) {
    const long long aa = (long long)blockIdx.x * NT + threadIdx.x;
    if (aa >= L.nv || accept[aa] == 0) return;
    const int a = (int)aa, b = targets[aa];
    if (!in_range(b, L.nv)) return;
    int start, end, ic, c, id, d;
    L.range(a, start, end);
    if (!L.editable(a, start, end, b, ic, c, id, d)) return;
    const long long cc = L.corners[ic], cd = L.corners[id];
    faces[3 * (cc / 3) + (cc % 3 + 1) % 3] = d;               // b's place in (a, b, c)
    faces[3 * (cd / 3) + cd % 3] = c;                         // a's place in (b, a, d)
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Relax: the umbrella step of meshtopo.hip's smooth pass without its part along the vertex normal of meshtopo.hip's normals
__global__ void __launch_bounds__(NT) remesh_relax_kernel(const float* __restrict__ verts_in, Lists L, const int32_t* __restrict__ boundary,
                                                          const int32_t* __restrict__ pinned, float lambda, float* __restrict__ verts_out) {
    const long long v = (long long)blockIdx.x * NT + threadIdx.x;
    if (v >= L.nv) return;
    const float px = verts_in[3 * v], py = verts_in[3 * v + 1], pz = verts_in[3 * v + 2];
    float ox = px, oy = py, oz = pz;
    if (boundary[v] == 0 && (pinned == nullptr || pinned[v] == 0)) {
        int start, end;
        L.range(v, start, end);
        float sx = 0.f, sy = 0.f, sz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
        int count = 0;
        for (int i = start; i < end; ++i) {
            int k, i0, i1, i2;
            if (!L.entry(i, k, i0, i1, i2)) continue;
            const long long a = corner_at(k, 1, i0, i1, i2), b = corner_at(k, 2, i0, i1, i2);
            sx += mul(0.5f, verts_in[3 * a] + verts_in[3 * b]);
            sy += mul(0.5f, verts_in[3 * a + 1] + verts_in[3 * b + 1]);
            sz += mul(0.5f, verts_in[3 * a + 2] + verts_in[3 * b + 2]);
            ++count;
            const float ax = verts_in[3 * (long long)i0], ay = verts_in[3 * (long long)i0 + 1], az = verts_in[3 * (long long)i0 + 2];
            const float ux = verts_in[3 * (long long)i1] - ax, uy = verts_in[3 * (long long)i1 + 1] - ay, uz = verts_in[3 * (long long)i1 + 2] - az;
            const float wx = verts_in[3 * (long long)i2] - ax, wy = verts_in[3 * (long long)i2 + 1] - ay, wz = verts_in[3 * (long long)i2 + 2] - az;
            nx += mul(uy, wz) - mul(uz, wy);
            ny += mul(uz, wx) - mul(ux, wz);
            nz += mul(ux, wy) - mul(uy, wx);
        }
        const float len2 = mul(nx, nx) + mul(ny, ny) + mul(nz, nz);
        if (count > 0 && len2 > 1e-20f) {
            const float len = sqrtf(len2), n = (float)count;
            nx /= len;
            ny /= len;
            nz /= len;
            const float dx = sx / n - px, dy = sy / n - py, dz = sz / n - pz;
            const float nd = (mul(nx, dx) + mul(ny, dy)) + mul(nz, dz);
            ox = px + mul(lambda, dx - mul(nx, nd));
            oy = py + mul(lambda, dy - mul(ny, nd));
            oz = pz + mul(lambda, dz - mul(nz, nd));
        }
    }
    verts_out[3 * v] = ox;
    verts_out[3 * v + 1] = oy;
    verts_out[3 * v + 2] = oz;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Reproject: vertex v moves to the point (hit_face, u, v) of the input mesh and takes the colour interpolated there
__device__ __forceinline__ float on_triangle(float a, float b, float c, float u, float v) {
    float q = a + mul(u, b - a) + mul(v, c - a);
    if (u == 1.f) q = b;                                      // a vertex is itself, not a + (b - a) rounded twice
    if (v == 1.f) q = c;
    return q;
}

__global__ void __launch_bounds__(NT) remesh_project_kernel(const int32_t* __restrict__ hit_face, const float* __restrict__ hit_uv,
                                                            const float* __restrict__ src_verts, const float* __restrict__ src_colors, int src_nv,
                                                            const int32_t* __restrict__ src_faces, int src_nf, float* __restrict__ verts,
                                                            float* __restrict__ colors, int nv) {
    const long long t = (long long)blockIdx.x * NT + threadIdx.x;
    if (t >= nv) return;
    const int f = hit_face[t];
    if (!in_range(f, src_nf)) return;                         // a miss keeps the vertex
    int i0, i1, i2;
    if (!load_face(src_faces, f, src_nv, i0, i1, i2)) return;
    const float u = hit_uv[2 * t], v = hit_uv[2 * t + 1];
    if (!(u >= 0.f && v >= 0.f && u <= 1.f && v <= 1.f)) return;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        verts[3 * t + j] = on_triangle(src_verts[3 * (long long)i0 + j], src_verts[3 * (long long)i1 + j], src_verts[3 * (long long)i2 + j], u, v);
        colors[3 * t + j] = on_triangle(src_colors[3 * (long long)i0 + j], src_colors[3 * (long long)i1 + j], src_colors[3 * (long long)i2 + j], u, v);
    }
}

bool edge_ok(float e) { return e > 0.f && e < INFINITY; }

}  // namespace

#define REMESH_REQUIRE_EDGE(name, e) RECON_REQUIRE(edge_ok(e), name ": target_edge %g must be positive and finite", (double)(e))

extern "C" int v3d_recon_remesh_split_propose(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                              const int32_t* corners, float target_edge, int32_t max_valence, uint64_t* keys, int32_t* targets,
                                              v3d_stream_t stream) {
    RECON_REQUIRE(verts && faces && ranges && corners && keys && targets, "v3d_recon_remesh_split_propose: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_remesh_split_propose", num_verts, num_faces);
    REMESH_REQUIRE_EDGE("v3d_recon_remesh_split_propose", target_edge);
    MESH_REQUIRE_VALENCE("v3d_recon_remesh_split_propose", max_valence);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    const float L2 = target_edge * target_edge, hi2 = (16.f / 9.f) * L2;
    hipLaunchKernelGGL(remesh_split_propose_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, verts, L, L2, hi2, (int)max_valence,
                       (unsigned long long*)keys, targets);
    return check_launch("v3d_recon_remesh_split_propose");
}

extern "C" int v3d_recon_remesh_split_apply(float* verts, float* colors, int32_t num_verts, int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                            const int32_t* corners, const int32_t* accept, const int32_t* targets, const int32_t* rank,
                                            const int32_t* counts_in, int32_t* counts_out, int32_t* flag, v3d_stream_t stream) {
    RECON_REQUIRE(verts && colors && faces && ranges && corners && accept && targets && rank && counts_in && counts_out && flag,
                  "v3d_recon_remesh_split_apply: null argument");
    RECON_REQUIRE(counts_in != counts_out, "v3d_recon_remesh_split_apply: counts_in and counts_out must be two buffers");
    MESH_REQUIRE_COUNTS("v3d_recon_remesh_split_apply", num_verts, num_faces);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(remesh_split_apply_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, verts, colors, faces, L, accept, targets, rank, counts_in,
                       counts_out, flag);
    return check_launch("v3d_recon_remesh_split_apply");
}

extern "C" int v3d_recon_remesh_collapse_propose(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                                 const int32_t* corners, float target_edge, int32_t max_valence, uint64_t* keys, int32_t* targets,
                                                 v3d_stream_t stream) {
    RECON_REQUIRE(verts && faces && ranges && corners && keys && targets, "v3d_recon_remesh_collapse_propose: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_remesh_collapse_propose", num_verts, num_faces);
    REMESH_REQUIRE_EDGE("v3d_recon_remesh_collapse_propose", target_edge);
    MESH_REQUIRE_VALENCE("v3d_recon_remesh_collapse_propose", max_valence);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    const float L2 = target_edge * target_edge, lo2 = (16.f / 25.f) * L2, hi2 = (16.f / 9.f) * L2;
    hipLaunchKernelGGL(remesh_collapse_propose_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, verts, L, lo2, hi2, (int)max_valence,
                       (unsigned long long*)keys, targets);
    return check_launch("v3d_recon_remesh_collapse_propose");
}

extern "C" int v3d_recon_remesh_collapse_apply(int32_t* faces, int32_t num_faces, int32_t num_verts, const int32_t* ranges, const int32_t* corners,
                                               const int32_t* accept, const int32_t* targets, int32_t* removed, v3d_stream_t stream) {
    RECON_REQUIRE(faces && ranges && corners && accept && targets && removed, "v3d_recon_remesh_collapse_apply: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_remesh_collapse_apply", num_verts, num_faces);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(remesh_collapse_apply_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, faces, L, accept, targets, removed);
    return check_launch("v3d_recon_remesh_collapse_apply");
}

extern "C" int v3d_recon_remesh_flip_propose(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                             const int32_t* corners, const int32_t* boundary, int32_t max_valence, uint64_t* keys, int32_t* targets,
                                             v3d_stream_t stream) {
    RECON_REQUIRE(verts && faces && ranges && corners && boundary && keys && targets, "v3d_recon_remesh_flip_propose: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_remesh_flip_propose", num_verts, num_faces);
    MESH_REQUIRE_VALENCE("v3d_recon_remesh_flip_propose", max_valence);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(remesh_flip_propose_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, verts, L, boundary, (int)max_valence,
                       (unsigned long long*)keys, targets);
    return check_launch("v3d_recon_remesh_flip_propose");
}

extern "C" int v3d_recon_remesh_flip_apply(int32_t* faces, int32_t num_faces, int32_t num_verts, const int32_t* ranges, const int32_t* corners,
                                           const int32_t* accept, const int32_t* targets, v3d_stream_t stream) {
    RECON_REQUIRE(faces && ranges && corners && accept && targets, "v3d_recon_remesh_flip_apply: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_remesh_flip_apply", num_verts, num_faces);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(remesh_flip_apply_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, faces, L, accept, targets);
    return check_launch("v3d_recon_remesh_flip_apply");
}

extern "C" int v3d_recon_remesh_relax(const float* verts_in, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                      const int32_t* corners, const int32_t* boundary, const int32_t* pinned, float lambda, float* verts_out,
                                      v3d_stream_t stream) {
    RECON_REQUIRE(verts_in && faces && ranges && corners && boundary && verts_out, "v3d_recon_remesh_relax: null argument");
    RECON_REQUIRE(verts_in != verts_out, "v3d_recon_remesh_relax: verts_in and verts_out must be two buffers");
    MESH_REQUIRE_COUNTS("v3d_recon_remesh_relax", num_verts, num_faces);
    RECON_REQUIRE(lambda >= 0.f && lambda <= 1.f, "v3d_recon_remesh_relax: lambda %g outside 0 .. 1", (double)lambda);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(remesh_relax_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, verts_in, L, boundary, pinned, lambda, verts_out);
    return check_launch("v3d_recon_remesh_relax");
}

extern "C" int v3d_recon_remesh_project(const int32_t* hit_face, const float* hit_uv, const float* src_verts, const float* src_colors,
                                        int32_t src_num_verts, const int32_t* src_faces, int32_t src_num_faces, float* verts, float* colors,
                                        int32_t num_verts, v3d_stream_t stream) {
    RECON_REQUIRE(hit_face && hit_uv && src_verts && src_colors && src_faces && verts && colors, "v3d_recon_remesh_project: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_remesh_project", src_num_verts, src_num_faces);
    RECON_REQUIRE(num_verts > 0, "v3d_recon_remesh_project: num_verts %d must be positive", (int)num_verts);
    RECON_REQUIRE(verts != src_verts && colors != src_colors, "v3d_recon_remesh_project: the input mesh and the vertices must be two buffers");
    hipLaunchKernelGGL(remesh_project_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, hit_face, hit_uv, src_verts, src_colors, (int)src_num_verts,
                       src_faces, (int)src_num_faces, verts, colors, (int)num_verts);
    return check_launch("v3d_recon_remesh_project");
}
