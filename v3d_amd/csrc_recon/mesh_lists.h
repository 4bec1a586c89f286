// Shared by the sources of libv3d_recon.so that walk the vertex -> incident-corner lists (meshtopo.hip, meshdecim.hip, meshremesh.hip): the
// face loader, the walk over one vertex's list (struct Lists), the two integer rules every half-edge collapse v -> u obeys (v's star is one
// closed fan; the collapse leaves a manifold behind), the fp64 position loader, and the host checks behind the entries that take the lists.
// The lists come from corner_records -> v3d_gs_radix_sort_pairs -> v3d_recon_mesh_vertex_ranges, rebuilt by the host whenever the faces
// change.  Everything here is integers or a plain load: the arithmetic of a stage (its cross products, its rounding) stays in its source.
// Everything sits in an anonymous namespace: every source that includes this gets its own copy, as when the code stood in the source itself.
#ifndef V3D_RECON_MESH_LISTS_H
#define V3D_RECON_MESH_LISTS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "recon_host.h"
#include "v3d_recon.h"

namespace {

constexpr unsigned long long NO_KEY = ~0ull;                  // the key of a vertex that proposes nothing

__device__ __forceinline__ bool in_range(int i, int n) { return i >= 0 && i < n; }

// The three vertices of face f; false when one of them lies outside 0 .. nv-1 (the face is then absent)
__device__ __forceinline__ bool load_face(const int32_t* faces, long long f, int nv, int& i0, int& i1, int& i2) {
    i0 = faces[3 * f];
    i1 = faces[3 * f + 1];
    i2 = faces[3 * f + 2];
    return in_range(i0, nv) && in_range(i1, nv) && in_range(i2, nv);
}

// Corner (k + s) % 3 of a face, without an indexed array
__device__ __forceinline__ int corner_at(int k, int s, int i0, int i1, int i2) {
    const int j = (k + s) % 3;
    return j == 0 ? i0 : (j == 1 ? i1 : i2);
}

// The walk over one vertex's list: entry i gives the face's three vertices, the corner's place k, and the two neighbours a = next, b = prev.
// (faces is not __restrict__: the apply kernels of meshremesh.hip write the faces they have read through it)
struct Lists {
    const int32_t* faces;
    const int32_t* __restrict__ ranges;
    const int32_t* __restrict__ corners;
    int nf, nv;

    // the clamped [start, end) of vertex v's list
    __device__ __forceinline__ void range(long long v, int& start, int& end) const {
        start = max(ranges[2 * v], 0);
        end = (int)min((long long)ranges[2 * v + 1], 3LL * nf);
    }
    // the face of corner corners[i] and the corner's place k in it; false for a corner outside 0 .. 3F-1 or an absent face
    __device__ __forceinline__ bool entry(int i, int& k, int& i0, int& i1, int& i2) const {
        const long long c = corners[i];
        if (c < 0 || c >= 3LL * nf) return false;
        k = (int)(c % 3);
        return load_face(faces, c / 3, nv, i0, i1, i2);
    }
    __device__ __forceinline__ bool neighbours(int i, int& a, int& b) const {
        int k, i0, i1, i2;
        if (!entry(i, k, i0, i1, i2)) return false;
        a = corner_at(k, 1, i0, i1, i2);
        b = corner_at(k, 2, i0, i1, i2);
        return true;
    }
    // present entries of the list, counted up to limit + 1
    __device__ __forceinline__ int count(int start, int end, int limit) const {
        int n = 0;
        for (int i = start; i < end && n <= limit; ++i) {
            int a, b;
            n += neighbours(i, a, b) ? 1 : 0;
        }
        return n;
    }
    __device__ __forceinline__ int valence(int v, int limit) const {
        int s, e;
        range(v, s, e);
        return count(s, e, limit);
    }
    // The edge (a, b) from a's list [start, end): editable when exactly one entry has b next (the face a b c, entry ic) and exactly one has b
    // before a (the face b a d, entry id), and a, b, c, d are four vertices
    __device__ __forceinline__ bool editable(int a, int start, int end, int b, int& ic, int& c, int& id, int& d) const {
        int nab = 0, nba = 0;
        ic = id = c = d = -1;
        for (int i = start; i < end; ++i) {
            int x, y;
            if (!neighbours(i, x, y)) continue;
            if (x == b) {
                ++nab;
                ic = i;
                c = y;
            }
            if (y == b) {
                ++nba;
                id = i;
                d = x;
            }
        }
        return nab == 1 && nba == 1 && b != a && c != d && c != a && d != a && c != b && d != b;
    }
};

// ---------------------------------------------------------------------------------------------------------------------------------------
// Is v's star [start, end), of n_v present entries, one closed fan?
__device__ __forceinline__ bool closed_fan(const Lists& L, int v, int start, int end, int n_v) {
    bool removable = true;
    // a closed fan: every neighbour is the next corner of one entry and the previous corner of one entry ..
    for (int i = start; i < end && removable; ++i) {
        int a, b;
        if (!L.neighbours(i, a, b)) continue;
        if (a == v || b == v || a == b) removable = false;
        int na = 0, pa = 0, nb = 0, pb = 0;
        for (int j = start; j < end; ++j) {
            int x, y;
            if (!L.neighbours(j, x, y)) continue;
            na += x == a;
            pa += y == a;
            nb += x == b;
            pb += y == b;
        }
        removable = removable && na == 1 && pa == 1 && nb == 1 && pb == 1;
    }
    // .. and one fan, not several that meet at v: stepping from an entry to the one that starts where it ends comes round after n_v steps
    if (removable) {
        int first = -1, x = -1, steps = 0;
        for (int i = start; i < end && first < 0; ++i) {
            int a, b;
            if (L.neighbours(i, a, b)) {
                first = a;
                x = b;
            }
        }
        for (steps = 1; steps <= n_v && x != first; ++steps) {
            int nx = first;
            for (int j = start; j < end; ++j) {
                int a, b;
                if (L.neighbours(j, a, b) && a == x) nx = b;
            }
            x = nx;
        }
        removable = steps == n_v;
    }
    return removable;
}

// Does v -> u leave a manifold behind, given that v's star [start, end) is one closed fan of n_v faces?  i_u: the entry of v's list whose
// next neighbour is u.  The integer half of a collapse's validity; what depends on positions is the calling stage's own.
__device__ __forceinline__ bool collapse_topology_ok(const Lists& L, int v, int start, int end, int n_v, int u, int i_u, int max_valence) {
    int a1, a2 = -1, t;
    L.neighbours(i_u, t, a1);                                 // the face (v, u, a1)
    for (int j = start; j < end; ++j) {                       // the face (v, a2, u)
        int a, b;
        if (L.neighbours(j, a, b) && b == u) a2 = a;
    }
    if (a2 < 0 || a1 == a2) return false;
    int us, ue;
    L.range(u, us, ue);
    const int room = max_valence + 4 - n_v;                   // u ends with n_u + n_v - 4 faces
    if (L.count(us, ue, room) > room) return false;
    // the link condition: no neighbour of v other than the two apexes is a neighbour of u
    for (int j = start; j < end; ++j) {
        int w, b;
        if (!L.neighbours(j, w, b) || w == u || w == a1 || w == a2) continue;
        for (int m = us; m < ue; ++m) {
            int x, y;
            if (L.neighbours(m, x, y) && (x == w || y == w)) return false;
        }
    }
    for (int j = start; j < end; ++j) {                       // the faces that survive: v's faces without u
        int a, b;
        if (!L.neighbours(j, a, b) || a == u || b == u) continue;
        for (int m = us; m < ue; ++m) {                       // u already has a face on these three vertices
            int x, y;
            if (L.neighbours(m, x, y) && ((x == a && y == b) || (x == b && y == a))) return false;
        }
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
struct D3 {
    double x, y, z;
};

__device__ __forceinline__ D3 load_pos(const float* __restrict__ verts, long long i) {
    return D3{(double)verts[3 * i], (double)verts[3 * i + 1], (double)verts[3 * i + 2]};
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Host side of the entries that take the lists
inline bool counts_ok(int32_t nv, int32_t nf) { return nv > 0 && nf > 0 && nf <= INT32_MAX / 3; }

}  // namespace

#define ST ((hipStream_t)stream)
#define MESH_REQUIRE_COUNTS(name, nv, nf)                                                                                              \
    RECON_REQUIRE(counts_ok(nv, nf), name ": num_verts %d and num_faces %d must be positive, 3 x num_faces at most INT32_MAX", (int)(nv), \
                  (int)(nf))
#define MESH_REQUIRE_VALENCE(name, m) \
    RECON_REQUIRE((m) >= 3 && (m) <= V3D_RECON_MESH_MAX_VALENCE, name ": max_valence %d outside 3 .. %d", (int)(m), V3D_RECON_MESH_MAX_VALENCE)

#endif
