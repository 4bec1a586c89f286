// The extracted mesh as a graph (include/v3d_recon.h "Mesh topology", libv3d_recon.so; host side: v3d_amd/recon/mesh_clean.py): the
// vertex -> incident-corner lists, and what walks them: area-weighted vertex normals, connected components by min-label propagation with one
// pointer jump per round, the flags and the index remap of the component filter, open-edge (boundary) flags and one pass of umbrella
// smoothing.  The lists come from corner_records -> v3d_gs_radix_sort_pairs -> v3d_recon_mesh_vertex_ranges (meshshade.hip); the scans and the
// sorts are libv3d_hip.so's, called by the host.  The walk itself (struct Lists) is mesh_lists.h's, shared with meshdecim.hip and
// meshremesh.hip.
//
// No atomics: every output element belongs to one thread, which walks its vertex's list in list order (ascending corner index, the sort is
// stable), so every sum has one order and two runs are bit-equal.  Lists are short (valence 4 - 10 on what surface nets produce): one thread
// per vertex, no wave-wide reduction.  A face with an index outside 0 .. V-1 is absent everywhere: no kernel reads through such an index.
// Built without -ffast-math (v3d_amd/build.py), and without contraction: a sum of products is rounded as the float32 run of the restatement
// (tests/mesh_clean_ref.py) rounds it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mesh_lists.h"
#include "recon_host.h"
#include "v3d_recon.h"

#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------------------------------------------------------------------------------
// Three records per face in face order: the stable sort on the vertex leaves every vertex's corners in ascending 3 f + k.  A record whose
// vertex is out of range goes to vertex 0 (the key must stay inside the sorted bits); whoever walks the list finds its face absent.
__global__ void __launch_bounds__(NT) mesh_corner_records_kernel(const int32_t* __restrict__ faces, long long n, int nv,
                                                                 unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
    const long long c = (long long)blockIdx.x * NT + threadIdx.x;
    if (c >= n) return;
    const int v = faces[c];
    keys[c] = in_range(v, nv) ? (unsigned long long)v : 0ull;
    vals[c] = (uint32_t)c;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) mesh_vertex_normals_kernel(const float* __restrict__ verts, Lists L, float* __restrict__ normals) {
    const long long v = (long long)blockIdx.x * NT + threadIdx.x;
    if (v >= L.nv) return;
    int start, end;
    L.range(v, start, end);
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int i = start; i < end; ++i) {
        int k, i0, i1, i2;
        if (!L.entry(i, k, i0, i1, i2)) continue;
        const float ax = verts[3 * (long long)i0], ay = verts[3 * (long long)i0 + 1], az = verts[3 * (long long)i0 + 2];
        const float ux = verts[3 * (long long)i1] - ax, uy = verts[3 * (long long)i1 + 1] - ay, uz = verts[3 * (long long)i1 + 2] - az;
        const float wx = verts[3 * (long long)i2] - ax, wy = verts[3 * (long long)i2 + 1] - ay, wz = verts[3 * (long long)i2 + 2] - az;
        nx += uy * wz - uz * wy;
        ny += uz * wx - ux * wz;
        nz += ux * wy - uy * wx;
    }
    const float len2 = nx * nx + ny * ny + nz * nz;
    if (len2 > 1e-20f) {
        const float len = sqrtf(len2);
        nx /= len;
        ny /= len;
        nz /= len;
    } else {                                      // no face, faces without area, or normals that cancel
        nx = 0.f;
        ny = 0.f;
        nz = 1.f;
    }
    normals[3 * v] = nx;
    normals[3 * v + 1] = ny;
    normals[3 * v + 2] = nz;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// One round of the labelling.  labels_in is read-only for the whole launch and labels_out has one owner per element, so the result does not
// depend on the order in which threads run.  Labels only ever fall, and stay inside the component: labels[x] <= x names a vertex joined to x.
__global__ void __launch_bounds__(NT) mesh_label_round_kernel(Lists L, const int32_t* __restrict__ labels_in, int32_t* __restrict__ labels_out,
                                                              int32_t* __restrict__ changed) {
    const long long v = (long long)blockIdx.x * NT + threadIdx.x;
    if (v >= L.nv) return;
    int start, end;
    L.range(v, start, end);
    const int mine = labels_in[v];
    int m = mine;
    for (int i = start; i < end; ++i) {
        int k, i0, i1, i2;
        if (!L.entry(i, k, i0, i1, i2)) continue;
        m = min(m, min(labels_in[i0], min(labels_in[i1], labels_in[i2])));
    }
    const int out = in_range(m, L.nv) ? labels_in[m] : mine;              // the jump (labels[m] <= m on labels this pass made)
    labels_out[v] = out;
    if (out != mine) *changed = 1;                                        // (every writer stores the same value)
}

// keys = the label of the face's first corner, vals = the face, in face order; an absent face gets the key nv, which no range counts
__global__ void __launch_bounds__(NT) mesh_face_labels_kernel(const int32_t* __restrict__ faces, int nf, const int32_t* __restrict__ labels, int nv,
                                                              unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
    const long long f = (long long)blockIdx.x * NT + threadIdx.x;
    if (f >= nf) return;
    int i0, i1, i2;
    unsigned long long key = (unsigned long long)nv;
    if (load_face(faces, f, nv, i0, i1, i2)) {
        const int l = labels[i0];
        if (in_range(l, nv)) key = (unsigned long long)l;
    }
    keys[f] = key;
    vals[f] = (uint32_t)f;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Thread t decides face t (t < nf) and vertex t (t < nv)
__global__ void __launch_bounds__(NT) mesh_keep_flags_kernel(Lists L, const int32_t* __restrict__ labels, const int32_t* __restrict__ keep_root,
                                                             int32_t* __restrict__ keep_face, int32_t* __restrict__ keep_vert) {
    const long long t = (long long)blockIdx.x * NT + threadIdx.x;
    if (t < L.nf) {
        int i0, i1, i2, keep = 0;
        if (load_face(L.faces, t, L.nv, i0, i1, i2)) {
            const int l = labels[i0];
            keep = in_range(l, L.nv) && keep_root[l] != 0;
        }
        keep_face[t] = keep;
    }
    if (t < L.nv) {
        const int l = labels[t];
        int keep = 0;
        if (in_range(l, L.nv) && keep_root[l] != 0) {
            int start, end;
            L.range(t, start, end);
            for (int i = start; i < end && !keep; ++i) {
                int k, i0, i1, i2;
                keep = L.entry(i, k, i0, i1, i2);
            }
        }
        keep_vert[t] = keep;
    }
}

__global__ void __launch_bounds__(NT) mesh_compact_faces_kernel(const int32_t* __restrict__ faces, int nf, int nv, const int32_t* __restrict__ keep_face,
                                                                const int32_t* __restrict__ face_off, const int32_t* __restrict__ keep_vert,
                                                                const int32_t* __restrict__ vert_off, int nf_out, int nv_out,
                                                                int32_t* __restrict__ faces_out) {
    const long long f = (long long)blockIdx.x * NT + threadIdx.x;
    if (f >= nf || keep_face[f] == 0) return;
    int i0, i1, i2;
    if (!load_face(faces, f, nv, i0, i1, i2)) return;
    const long long o = face_off[f];
    if (o < 0 || o >= nf_out) return;                                      // (never, with the offsets of these flags)
    for (int k = 0; k < 3; ++k) {
        const int i = corner_at(k, 0, i0, i1, i2);
        const int n = keep_vert[i] != 0 ? vert_off[i] : -1;
        faces_out[3 * o + k] = in_range(n, nv_out) ? n : 0;                // (a kept face has kept vertices: the 0 is never written)
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// An entry of v's list at corner k has the neighbours faces[f][(k + 1) % 3] and faces[f][(k + 2) % 3].  v lies on an open edge when some
// neighbour other than v is a neighbour in exactly one entry.  Quadratic in the list length, which is 4 - 10 here.
__global__ void __launch_bounds__(NT) mesh_boundary_flags_kernel(Lists L, int32_t* __restrict__ flags) {
    const long long v = (long long)blockIdx.x * NT + threadIdx.x;
    if (v >= L.nv) return;
    int start, end;
    L.range(v, start, end);
    int open = 0;
    for (int i = start; i < end && !open; ++i) {
        int k, i0, i1, i2;
        if (!L.entry(i, k, i0, i1, i2)) continue;
        for (int s = 1; s <= 2 && !open; ++s) {
            const int u = corner_at(k, s, i0, i1, i2);
            if (u == v) continue;
            int count = 0;
            for (int j = start; j < end && count < 2; ++j) {
                int kj, j0, j1, j2;
                if (!L.entry(j, kj, j0, j1, j2)) continue;
                count += (corner_at(kj, 1, j0, j1, j2) == u || corner_at(kj, 2, j0, j1, j2) == u) ? 1 : 0;
            }
            open = count == 1;
        }
    }
    flags[v] = open;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) mesh_smooth_pass_kernel(const float* __restrict__ verts_in, Lists L, const int32_t* __restrict__ pinned,
                                                              float factor, float* __restrict__ verts_out) {
    const long long v = (long long)blockIdx.x * NT + threadIdx.x;
    if (v >= L.nv) return;
    const float px = verts_in[3 * v], py = verts_in[3 * v + 1], pz = verts_in[3 * v + 2];
    float ox = px, oy = py, oz = pz;
    if (pinned == nullptr || pinned[v] == 0) {
        int start, end;
        L.range(v, start, end);
        float sx = 0.f, sy = 0.f, sz = 0.f;
        int count = 0;
        for (int i = start; i < end; ++i) {
            int k, i0, i1, i2;
            if (!L.entry(i, k, i0, i1, i2)) continue;
            const long long a = corner_at(k, 1, i0, i1, i2), b = corner_at(k, 2, i0, i1, i2);
            sx += 0.5f * (verts_in[3 * a] + verts_in[3 * b]);
            sy += 0.5f * (verts_in[3 * a + 1] + verts_in[3 * b + 1]);
            sz += 0.5f * (verts_in[3 * a + 2] + verts_in[3 * b + 2]);
            ++count;
        }
        if (count > 0) {
            const float n = (float)count;
            ox = px + factor * (sx / n - px);
            oy = py + factor * (sy / n - py);
            oz = pz + factor * (sz / n - pz);
        }
    }
    verts_out[3 * v] = ox;
    verts_out[3 * v + 1] = oy;
    verts_out[3 * v + 2] = oz;
}

}  // namespace

extern "C" int v3d_recon_mesh_corner_records(const int32_t* faces, int32_t num_faces, int32_t num_verts, uint64_t* keys, uint32_t* vals,
                                             v3d_stream_t stream) {
    RECON_REQUIRE(faces && keys && vals, "v3d_recon_mesh_corner_records: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_mesh_corner_records", num_verts, num_faces);
    hipLaunchKernelGGL(mesh_corner_records_kernel, dim3(nblk(3LL * num_faces)), dim3(NT), 0, ST, faces, 3LL * num_faces, (int)num_verts,
                       (unsigned long long*)keys, vals);
    return check_launch("v3d_recon_mesh_corner_records");
}

extern "C" int v3d_recon_mesh_vertex_normals(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                             const int32_t* corners, float* normals, v3d_stream_t stream) {
    RECON_REQUIRE(verts && faces && ranges && corners && normals, "v3d_recon_mesh_vertex_normals: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_mesh_vertex_normals", num_verts, num_faces);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(mesh_vertex_normals_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, verts, L, normals);
    return check_launch("v3d_recon_mesh_vertex_normals");
}

extern "C" int v3d_recon_mesh_label_round(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                                          const int32_t* labels_in, int32_t* labels_out, int32_t* changed, v3d_stream_t stream) {
    RECON_REQUIRE(faces && ranges && corners && labels_in && labels_out && changed, "v3d_recon_mesh_label_round: null argument");
    RECON_REQUIRE(labels_in != labels_out, "v3d_recon_mesh_label_round: labels_in and labels_out must be two buffers");
    MESH_REQUIRE_COUNTS("v3d_recon_mesh_label_round", num_verts, num_faces);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(mesh_label_round_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, L, labels_in, labels_out, changed);
    return check_launch("v3d_recon_mesh_label_round");
}

extern "C" int v3d_recon_mesh_face_labels(const int32_t* faces, int32_t num_faces, const int32_t* labels, int32_t num_verts, uint64_t* keys,
                                          uint32_t* vals, v3d_stream_t stream) {
    RECON_REQUIRE(faces && labels && keys && vals, "v3d_recon_mesh_face_labels: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_mesh_face_labels", num_verts, num_faces);
    hipLaunchKernelGGL(mesh_face_labels_kernel, dim3(nblk(num_faces)), dim3(NT), 0, ST, faces, (int)num_faces, labels, (int)num_verts,
                       (unsigned long long*)keys, vals);
    return check_launch("v3d_recon_mesh_face_labels");
}

extern "C" int v3d_recon_mesh_keep_flags(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                                         const int32_t* labels, const int32_t* keep_root, int32_t* keep_face, int32_t* keep_vert, v3d_stream_t stream) {
    RECON_REQUIRE(faces && ranges && corners && labels && keep_root && keep_face && keep_vert, "v3d_recon_mesh_keep_flags: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_mesh_keep_flags", num_verts, num_faces);
    const long long n = num_faces > num_verts ? num_faces : num_verts;
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(mesh_keep_flags_kernel, dim3(nblk(n)), dim3(NT), 0, ST, L, labels, keep_root, keep_face, keep_vert);
    return check_launch("v3d_recon_mesh_keep_flags");
}

extern "C" int v3d_recon_mesh_compact_faces(const int32_t* faces, int32_t num_faces, int32_t num_verts, const int32_t* keep_face, const int32_t* face_off,
                                            const int32_t* keep_vert, const int32_t* vert_off, int32_t num_faces_out, int32_t num_verts_out,
                                            int32_t* faces_out, v3d_stream_t stream) {
    RECON_REQUIRE(faces && keep_face && face_off && keep_vert && vert_off && faces_out, "v3d_recon_mesh_compact_faces: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_mesh_compact_faces", num_verts, num_faces);
    RECON_REQUIRE(num_faces_out > 0 && num_faces_out <= num_faces && num_verts_out > 0 && num_verts_out <= num_verts,
                  "v3d_recon_mesh_compact_faces: %d faces and %d vertices out of %d and %d", (int)num_faces_out, (int)num_verts_out, (int)num_faces,
                  (int)num_verts);
    hipLaunchKernelGGL(mesh_compact_faces_kernel, dim3(nblk(num_faces)), dim3(NT), 0, ST, faces, (int)num_faces, (int)num_verts, keep_face, face_off,
                       keep_vert, vert_off, (int)num_faces_out, (int)num_verts_out, faces_out);
    return check_launch("v3d_recon_mesh_compact_faces");
}

extern "C" int v3d_recon_mesh_boundary_flags(const int32_t* faces, int32_t num_faces, const int32_t* ranges, const int32_t* corners, int32_t num_verts,
                                             int32_t* flags, v3d_stream_t stream) {
    RECON_REQUIRE(faces && ranges && corners && flags, "v3d_recon_mesh_boundary_flags: null argument");
    MESH_REQUIRE_COUNTS("v3d_recon_mesh_boundary_flags", num_verts, num_faces);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(mesh_boundary_flags_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, L, flags);
    return check_launch("v3d_recon_mesh_boundary_flags");
}

extern "C" int v3d_recon_mesh_smooth_pass(const float* verts_in, int32_t num_verts, const int32_t* faces, int32_t num_faces, const int32_t* ranges,
                                          const int32_t* corners, const int32_t* pinned, float factor, float* verts_out, v3d_stream_t stream) {
    RECON_REQUIRE(verts_in && faces && ranges && corners && verts_out, "v3d_recon_mesh_smooth_pass: null argument");
    RECON_REQUIRE(verts_in != verts_out, "v3d_recon_mesh_smooth_pass: verts_in and verts_out must be two buffers");
    MESH_REQUIRE_COUNTS("v3d_recon_mesh_smooth_pass", num_verts, num_faces);
    RECON_REQUIRE(isfinite(factor), "v3d_recon_mesh_smooth_pass: factor %g is not finite", (double)factor);
    const Lists L{faces, ranges, corners, (int)num_faces, (int)num_verts};
    hipLaunchKernelGGL(mesh_smooth_pass_kernel, dim3(nblk(num_verts)), dim3(NT), 0, ST, verts_in, L, pinned, factor, verts_out);
    return check_launch("v3d_recon_mesh_smooth_pass");
}
