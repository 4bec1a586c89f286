// Tangent space of the per-face atlas (include/v3d_recon.h "Tangent space and GLB", libv3d_recon.so; host side: v3d_amd/recon/mesh_gltf.py):
// per-corner NORMAL / TANGENT frames as glTF 2.0 wants them, the object-space normal map of meshbvh.hip re-expressed in those frames and
// back, and a lit shade of one frozen view (the pix_tex / pix_tw of meshtex.hip) from exactly the data a GLB carries.
//
// The frame is the header's THE TANGENT FRAME; every kernel below forms (vN, vT, vB) with the one function frame_at, and decodes and
// encodes with the one pair decode / encode.
//
// No atomics, no LDS: a face, a texel and a pixel each belong to one thread.  Streaming kernels of a few loads per item.
// Built without -ffast-math (v3d_amd/build.py): everything is held to an fp64 restatement (tests/mesh_tangent_ref.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "recon_host.h"
#include "v3d_recon.h"

namespace {

constexpr float LEN2_EPS = 1e-20f;      // a squared length that is not above this has no direction
constexpr float DET_EPS = 1e-12f;       // |det| of a frame that cannot be inverted

struct V3 {
    float x, y, z;
};

__device__ __forceinline__ V3 ld3(const float* __restrict__ p, long long row) { return {p[3 * row], p[3 * row + 1], p[3 * row + 2]}; }
__device__ __forceinline__ void st3(float* __restrict__ p, long long row, V3 a) { p[3 * row] = a.x, p[3 * row + 1] = a.y, p[3 * row + 2] = a.z; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 scale(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 mix3(float b0, V3 a, float b1, V3 b, float b2, V3 c) {
    return {b0 * a.x + b1 * b.x + b2 * c.x, b0 * a.y + b1 * b.y + b2 * c.y, b0 * a.z + b1 * b.z + b2 * c.z};
}
// a / |a|; false (a untouched) where the squared length is not above 1e-20 (a NaN included)
__device__ __forceinline__ bool unit(V3& a) {
    const float l2 = dot(a, a);
    if (!(l2 > LEN2_EPS)) return false;
    const float l = sqrtf(l2);
    a = {a.x / l, a.y / l, a.z / l};
    return true;
}

struct Frame {
    V3 n, t, b;
};

// (vN, vT, vB) at barycentrics b of face f from its three corner rows
__device__ __forceinline__ Frame frame_at(const float* __restrict__ cn, const float* __restrict__ ct, long long f, float b0, float b1, float b2) {
    Frame fr;
    fr.n = mix3(b0, ld3(cn, 3 * f), b1, ld3(cn, 3 * f + 1), b2, ld3(cn, 3 * f + 2));
    const float* t = ct + 12 * f;
    fr.t = mix3(b0, V3{t[0], t[1], t[2]}, b1, V3{t[4], t[5], t[6]}, b2, V3{t[8], t[9], t[10]});
    fr.b = scale(cross(fr.n, fr.t), t[3]);
    return fr;
}

__device__ __forceinline__ V3 decode(const Frame& fr, V3 c) {
    V3 n = {c.x * fr.t.x + c.y * fr.b.x + c.z * fr.n.x, c.x * fr.t.y + c.y * fr.b.y + c.z * fr.n.y, c.x * fr.t.z + c.y * fr.b.z + c.z * fr.n.z};
    if (unit(n)) return n;
    n = fr.n;
    if (unit(n)) return n;
    return {0.f, 0.f, 1.f};
}

__device__ __forceinline__ V3 encode(const Frame& fr, V3 m) {
    const V3 bn = cross(fr.b, fr.n), nt = cross(fr.n, fr.t), tb = cross(fr.t, fr.b);
    const float det = dot(fr.t, bn);
    if (!isfinite(det) || fabsf(det) <= DET_EPS) return {0.f, 0.f, 1.f};
    V3 c = {dot(m, bn) / det, dot(m, nt) / det, dot(m, tb) / det};
    if (!isfinite(dot(c, c)) || !unit(c)) return {0.f, 0.f, 1.f};
    return c;
}

__device__ __forceinline__ bool face_ok(const int32_t* __restrict__ faces, long long f, int nv, int& v0, int& v1, int& v2) {
    v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
    return v0 >= 0 && v0 < nv && v1 >= 0 && v1 < nv && v2 >= 0 && v2 < nv;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) corner_frames_kernel(const float* __restrict__ verts, int nv, const int32_t* __restrict__ faces, int nf,
                                                           const float* __restrict__ normals, float* __restrict__ cn, float* __restrict__ ct) {
    const long long f = (long long)blockIdx.x * NT + threadIdx.x;
    if (f >= nf) return;
    int idx[3];
    const bool ok = face_ok(faces, f, nv, idx[0], idx[1], idx[2]);
    V3 se1 = {0.f, 0.f, 0.f};
    if (ok) {
        const V3 p0 = ld3(verts, idx[0]), p1 = ld3(verts, idx[1]);
        const float s = (f & 1) ? -1.f : 1.f;
        se1 = {s * (p1.x - p0.x), s * (p1.y - p0.y), s * (p1.z - p0.z)};
    }
    for (int k = 0; k < 3; ++k) {
        V3 n = {0.f, 0.f, 1.f}, t = {1.f, 0.f, 0.f};
        if (ok) {
            n = ld3(normals, idx[k]);
            if (!unit(n)) n = {0.f, 0.f, 1.f};
            const float d = dot(n, se1);
            t = {se1.x - n.x * d, se1.y - n.y * d, se1.z - n.z * d};
            if (!unit(t)) {                                        // e1 along N (or no e1): the t1 of the occlusion kernel's basis
                const float q = copysignf(1.f, n.z), a = -1.f / (q + n.z), b = n.x * n.y * a;
                t = {1.f + q * n.x * n.x * a, q * b, -q * n.x};
            }
        }
        st3(cn, 3 * f + k, n);
        float* o = ct + 4 * (3 * f + k);
        o[0] = t.x, o[1] = t.y, o[2] = t.z, o[3] = -1.f;
    }
}

struct Atlas {
    int R, S, g, F;
};

// The owner and the barycentrics of texel t, exactly as tex_bake_kernel (meshtex.hip) forms them; -1 when unowned
__device__ __forceinline__ long long texel_owner(const Atlas& a, long long t, float& b0, float& b1, float& b2) {
    const int x = (int)(t % a.R), y = (int)(t / a.R);
    if (x >= a.g * a.S || y >= a.g * a.S) return -1;
    const int cx = x / a.S, cy = y / a.S;
    int i = x - cx * a.S, j = y - cy * a.S;
    const int half = i + j <= a.S - 2 ? 0 : 1;
    const long long f = 2LL * ((long long)cy * a.g + cx) + half;
    if (f >= a.F) return -1;
    if (half) i = a.S - 1 - i, j = a.S - 1 - j;
    const float L = (float)(a.S - 3);
    b1 = fminf(fmaxf((float)i / L, 0.f), 1.f);
    b2 = fminf(fmaxf((float)j / L, 0.f), 1.f - b1);
    b0 = 1.f - b1 - b2;
    return f;
}

template <bool ENCODE>
__global__ void __launch_bounds__(NT) texel_convert_kernel(Atlas a, const int32_t* __restrict__ faces, int nv, const float* __restrict__ cn,
                                                           const float* __restrict__ ct, const float* __restrict__ in, int32_t* __restrict__ owner,
                                                           float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * NT + threadIdx.x;
    if (t >= (long long)a.R * a.R) return;
    float b0, b1, b2;
    const long long f = texel_owner(a, t, b0, b1, b2);
    V3 r = {0.f, 0.f, 1.f};
    int v0, v1, v2;
    if (f >= 0 && face_ok(faces, f, nv, v0, v1, v2)) {
        const Frame fr = frame_at(cn, ct, f, b0, b1, b2);
        r = ENCODE ? encode(fr, ld3(in, t)) : decode(fr, ld3(in, t));
    }
    owner[t] = (int32_t)f;
    st3(out, t, r);
}

struct Lights {
    int K;
    float dir[V3D_RECON_LIT_MAX_LIGHTS][3];
    float intensity[V3D_RECON_LIT_MAX_LIGHTS];
};

__global__ void __launch_bounds__(NT) shade_lit_kernel(const int32_t* __restrict__ face_id, const float* __restrict__ pix_w,
                                                       const int32_t* __restrict__ pix_tex, const float* __restrict__ pix_tw, int nf,
                                                       const float* __restrict__ cn, const float* __restrict__ ct, const float* __restrict__ tmap,
                                                       const float* __restrict__ albedo, const float* __restrict__ ao_map, int nt, long long HW,
                                                       Lights lights, float ambient, float bg0, float bg1, float bg2, float* __restrict__ image,
                                                       float* __restrict__ normals) {
    const long long pix = (long long)blockIdx.x * NT + threadIdx.x;
    if (pix >= HW) return;
    float c0 = bg0, c1 = bg1, c2 = bg2;
    V3 n = {0.f, 0.f, 0.f};
    const int f = face_id[pix];
    const float w0 = pix_w[3 * pix], w1 = pix_w[3 * pix + 1], w2 = pix_w[3 * pix + 2];
    const float sum = w0 + w1 + w2;
    const int t0 = pix_tex[4 * pix], t1 = pix_tex[4 * pix + 1], t2 = pix_tex[4 * pix + 2], t3 = pix_tex[4 * pix + 3];
    if (f >= 0 && f < nf && sum > 0.f && t0 >= 0 && t0 < nt && t1 >= 0 && t1 < nt && t2 >= 0 && t2 < nt && t3 >= 0 && t3 < nt) {
        const float q0 = pix_tw[4 * pix], q1 = pix_tw[4 * pix + 1], q2 = pix_tw[4 * pix + 2], q3 = pix_tw[4 * pix + 3];
        const Frame fr = frame_at(cn, ct, f, w0 / sum, w1 / sum, w2 / sum);
        V3 c = {0.f, 0.f, 1.f};
        if (tmap) {
            const V3 a = ld3(tmap, t0), b = ld3(tmap, t1), d = ld3(tmap, t2), e = ld3(tmap, t3);
            c = {q0 * a.x + q1 * b.x + q2 * d.x + q3 * e.x, q0 * a.y + q1 * b.y + q2 * d.y + q3 * e.y, q0 * a.z + q1 * b.z + q2 * d.z + q3 * e.z};
        }
        n = decode(fr, c);
        float light = ambient * (ao_map ? q0 * ao_map[t0] + q1 * ao_map[t1] + q2 * ao_map[t2] + q3 * ao_map[t3] : 1.f);
        for (int k = 0; k < lights.K; ++k)
            light += lights.intensity[k] * fmaxf(0.f, dot(n, V3{lights.dir[k][0], lights.dir[k][1], lights.dir[k][2]}));
        const V3 a = ld3(albedo, t0), b = ld3(albedo, t1), d = ld3(albedo, t2), e = ld3(albedo, t3);
        c0 = (q0 * a.x + q1 * b.x + q2 * d.x + q3 * e.x) * light;
        c1 = (q0 * a.y + q1 * b.y + q2 * d.y + q3 * e.y) * light;
        c2 = (q0 * a.z + q1 * b.z + q2 * d.z + q3 * e.z) * light;
    }
    image[pix] = c0, image[HW + pix] = c1, image[2 * HW + pix] = c2;
    normals[pix] = n.x, normals[HW + pix] = n.y, normals[2 * HW + pix] = n.z;
}

bool image_ok(int32_t w, int32_t h) { return w > 0 && h > 0 && w <= V3D_RECON_MESH_MAX_IMAGE && h <= V3D_RECON_MESH_MAX_IMAGE; }

// g = ceil(sqrt(ceil(F / 2))), S = floor(R / g); false when a cell would be smaller than 4 texels (as meshtex.hip)
bool atlas_of(int32_t F, int32_t R, Atlas* a) {
    const long long cells = ((long long)F + 1) / 2;
    long long g = (long long)ceil(sqrt((double)cells));
    while (g * g < cells) ++g;
    while (g > 1 && (g - 1) * (g - 1) >= cells) --g;
    a->R = R, a->F = F, a->g = (int)g, a->S = (int)(R / g);
    return a->S >= V3D_RECON_TEX_MIN_CELL;
}

}  // namespace

#define ST ((hipStream_t)stream)
#define TAN_REQUIRE_ATLAS(name, F, R, a)                                                                                                            \
    RECON_REQUIRE((F) > 0, name ": num_faces must be positive");                                                                                    \
    RECON_REQUIRE((R) >= 1 && (R) <= V3D_RECON_TEX_MAX_SIZE, name ": tex_size %d outside 1 .. %d", (int)(R), V3D_RECON_TEX_MAX_SIZE);              \
    RECON_REQUIRE(atlas_of(F, R, &(a)), name ": texture too small for %d faces: %d x %d leaves cells of %d texels, below %d", (int)(F), (int)(R), \
                  (int)(R), (a).S, V3D_RECON_TEX_MIN_CELL)

extern "C" int v3d_recon_tex_corner_frames(const float* verts, int32_t num_verts, const int32_t* faces, int32_t num_faces, const float* normals,
                                           float* corner_normals, float* corner_tangents, v3d_stream_t stream) {
    RECON_REQUIRE(verts && faces && normals && corner_normals && corner_tangents, "v3d_recon_tex_corner_frames: null argument");
    RECON_REQUIRE(num_verts > 0, "v3d_recon_tex_corner_frames: num_verts must be positive");
    RECON_REQUIRE(num_faces > 0 && num_faces <= INT32_MAX / 3, "v3d_recon_tex_corner_frames: num_faces %d outside 1 .. %d (3 F must fit int32)",
                  (int)num_faces, INT32_MAX / 3);
    hipLaunchKernelGGL(corner_frames_kernel, dim3(nblk(num_faces)), dim3(NT), 0, ST, verts, (int)num_verts, faces, (int)num_faces, normals, corner_normals,
                       corner_tangents);
    return check_launch("v3d_recon_tex_corner_frames");
}

extern "C" int v3d_recon_tex_encode_tangent(const int32_t* faces, int32_t num_faces, int32_t num_verts, const float* corner_normals,
                                            const float* corner_tangents, const float* object_map, int32_t tex_size, int32_t* owner, float* tangent_map,
                                            v3d_stream_t stream) {
    Atlas a;
    RECON_REQUIRE(faces && corner_normals && corner_tangents && object_map && owner && tangent_map, "v3d_recon_tex_encode_tangent: null argument");
    RECON_REQUIRE(num_verts > 0, "v3d_recon_tex_encode_tangent: num_verts must be positive");
    TAN_REQUIRE_ATLAS("v3d_recon_tex_encode_tangent", num_faces, tex_size, a);
    hipLaunchKernelGGL(texel_convert_kernel<true>, dim3(nblk((long long)tex_size * tex_size)), dim3(NT), 0, ST, a, faces, (int)num_verts, corner_normals,
                       corner_tangents, object_map, owner, tangent_map);
    return check_launch("v3d_recon_tex_encode_tangent");
}

extern "C" int v3d_recon_tex_decode_tangent(const int32_t* faces, int32_t num_faces, int32_t num_verts, const float* corner_normals,
                                            const float* corner_tangents, const float* tangent_map, int32_t tex_size, int32_t* owner, float* object_map,
                                            v3d_stream_t stream) {
    Atlas a;
    RECON_REQUIRE(faces && corner_normals && corner_tangents && tangent_map && owner && object_map, "v3d_recon_tex_decode_tangent: null argument");
    RECON_REQUIRE(num_verts > 0, "v3d_recon_tex_decode_tangent: num_verts must be positive");
    TAN_REQUIRE_ATLAS("v3d_recon_tex_decode_tangent", num_faces, tex_size, a);
    hipLaunchKernelGGL(texel_convert_kernel<false>, dim3(nblk((long long)tex_size * tex_size)), dim3(NT), 0, ST, a, faces, (int)num_verts, corner_normals,
                       corner_tangents, tangent_map, owner, object_map);
    return check_launch("v3d_recon_tex_decode_tangent");
}

extern "C" int v3d_recon_tex_shade_lit(const int32_t* face_id, const float* pix_w, const int32_t* pix_tex, const float* pix_tw, int32_t num_faces,
                                       const float* corner_normals, const float* corner_tangents, const float* tangent_map, const float* albedo,
                                       const float* ao_map, int32_t tex_size, int32_t width, int32_t height, int32_t num_lights, const float* light_dirs,
                                       const float* light_intensity, float ambient, float bg0, float bg1, float bg2, float* image, float* normals,
                                       v3d_stream_t stream) {
    RECON_REQUIRE(face_id && pix_w && pix_tex && pix_tw && corner_normals && corner_tangents && albedo && image && normals,
                  "v3d_recon_tex_shade_lit: null argument");
    RECON_REQUIRE(num_faces > 0 && num_faces <= INT32_MAX / 3, "v3d_recon_tex_shade_lit: num_faces %d outside 1 .. %d", (int)num_faces, INT32_MAX / 3);
    RECON_REQUIRE(tex_size >= 1 && tex_size <= V3D_RECON_TEX_MAX_SIZE, "v3d_recon_tex_shade_lit: tex_size %d outside 1 .. %d", (int)tex_size,
                  V3D_RECON_TEX_MAX_SIZE);
    Atlas a;
    RECON_REQUIRE(atlas_of(num_faces, tex_size, &a), "v3d_recon_tex_shade_lit: texture too small for %d faces: %d x %d leaves cells of %d texels, below %d",
                  (int)num_faces, (int)tex_size, (int)tex_size, a.S, V3D_RECON_TEX_MIN_CELL);
    RECON_REQUIRE(image_ok(width, height), "v3d_recon_tex_shade_lit: image %d x %d outside 1 .. %d on a side", (int)width, (int)height,
                  V3D_RECON_MESH_MAX_IMAGE);
    RECON_REQUIRE(num_lights >= 0 && num_lights <= V3D_RECON_LIT_MAX_LIGHTS, "v3d_recon_tex_shade_lit: num_lights %d outside 0 .. %d", (int)num_lights,
                  V3D_RECON_LIT_MAX_LIGHTS);
    RECON_REQUIRE(num_lights == 0 || (light_dirs && light_intensity), "v3d_recon_tex_shade_lit: null light arrays with num_lights %d", (int)num_lights);
    Lights lights;
    memset(&lights, 0, sizeof(lights));
    lights.K = num_lights;
    for (int k = 0; k < num_lights; ++k) {
        for (int c = 0; c < 3; ++c) lights.dir[k][c] = light_dirs[3 * k + c];
        lights.intensity[k] = light_intensity[k];
    }
    const long long HW = (long long)width * height;
    hipLaunchKernelGGL(shade_lit_kernel, dim3(nblk(HW)), dim3(NT), 0, ST, face_id, pix_w, pix_tex, pix_tw, (int)num_faces, corner_normals, corner_tangents,
                       tangent_map, albedo, ao_map, (int)(tex_size * tex_size), HW, lights, ambient, bg0, bg1, bg2, image, normals);
    return check_launch("v3d_recon_tex_shade_lit");
}
