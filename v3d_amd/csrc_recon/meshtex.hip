// Texture of the decimated mesh (include/v3d_recon.h "Mesh texture", libv3d_recon.so; host side: v3d_amd/recon/mesh_texture.py).  The method
// of meshshade.hip with texels in the place of vertices: the geometry is fixed, so every view is rasterized once (meshrast.hip) and frozen
// into four texel indices and four bilinear weights per pixel (pixel_texels).  The image is a gather per pixel (shade), the gradient with
// respect to the texture the transposed gather per texel (shade_bwd) over lists that texel_records -> v3d_gs_radix_sort_pairs ->
// v3d_recon_mesh_vertex_ranges built once.  The optimiser's step is v3d_recon_mesh_color_adam on [R*R][3].
//
// The atlas is closed-form (the header states it): face f owns a right triangle of texels in cell f >> 1, so a texel's face (bake) and a
// face's UVs (face_uvs, pixel_texels) are integer arithmetic on the face index.
//
// No atomics: a face, a texel, a pixel and a record each belong to one thread; a texel's thread adds its list front to back.
// Built without -ffast-math (v3d_amd/build.py): everything is held to an fp64 restatement (tests/mesh_texture_ref.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "recon_host.h"
#include "v3d_recon.h"

namespace {

struct Atlas {
    int R, S, g, F;
};

// Where face f lives: its cell's origin, its half, and the last texel `hi` of the chart's bounding box (the same for x and y, relative to
// the cell's origin; the box starts at hi - L).
struct Chart {
    int x0, y0, half, hi;
};

__device__ __forceinline__ Chart chart_of(const Atlas& a, int f) {
    const int c = f >> 1;
    Chart ch;
    ch.x0 = (c % a.g) * a.S;
    ch.y0 = (c / a.g) * a.S;
    ch.half = f & 1;
    ch.hi = ch.half ? a.S - 1 : a.S - 3;
    return ch;
}

// corner `place` of the chart, in texels
__device__ __forceinline__ void corner_of(const Atlas& a, const Chart& ch, int place, float& u, float& v) {
    const int L = a.S - 3;
    const int dx = place == 1 ? L : 0, dy = place == 2 ? L : 0;
    u = (float)(ch.half ? ch.x0 + a.S - 1 - dx : ch.x0 + dx);
    v = (float)(ch.half ? ch.y0 + a.S - 1 - dy : ch.y0 + dy);
}

__global__ void __launch_bounds__(NT) tex_face_uvs_kernel(Atlas a, float* __restrict__ vt) {
    const long long fl = (long long)blockIdx.x * NT + threadIdx.x;
    if (fl >= a.F) return;
    const Chart ch = chart_of(a, (int)fl);
    for (int k = 0; k < 3; ++k) {
        float u, v;
        corner_of(a, ch, k, u, v);
        vt[6 * fl + 2 * k] = u;
        vt[6 * fl + 2 * k + 1] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Owner and initial albedo of every texel: the vertex colours, interpolated over the chart and held constant across its gutter.
__global__ void __launch_bounds__(NT) tex_bake_kernel(Atlas a, const int32_t* __restrict__ faces, const float* __restrict__ colors, int nv, float fill,
                                                      int32_t* __restrict__ owner, float* __restrict__ texture) {
    const long long t = (long long)blockIdx.x * NT + threadIdx.x;
    if (t >= (long long)a.R * a.R) return;
    const int x = (int)(t % a.R), y = (int)(t / a.R);
    int f = -1;
    float c0 = fill, c1 = fill, c2 = fill;
    if (x < a.g * a.S && y < a.g * a.S) {
        const int cx = x / a.S, cy = y / a.S;
        int i = x - cx * a.S, j = y - cy * a.S;
        const int half = i + j <= a.S - 2 ? 0 : 1;
        const long long fl = 2LL * ((long long)cy * a.g + cx) + half;
        if (fl < a.F) {
            f = (int)fl;
            if (half) i = a.S - 1 - i, j = a.S - 1 - j;
            const int v0 = faces[3 * fl], v1 = faces[3 * fl + 1], v2 = faces[3 * fl + 2];
            if (v0 >= 0 && v0 < nv && v1 >= 0 && v1 < nv && v2 >= 0 && v2 < nv) {
                const float L = (float)(a.S - 3);
                const float b1 = fminf(fmaxf((float)i / L, 0.f), 1.f);
                const float b2 = fminf(fmaxf((float)j / L, 0.f), 1.f - b1);
                const float b0 = 1.f - b1 - b2;
                c0 = b0 * colors[3 * (long long)v0] + b1 * colors[3 * (long long)v1] + b2 * colors[3 * (long long)v2];
                c1 = b0 * colors[3 * (long long)v0 + 1] + b1 * colors[3 * (long long)v1 + 1] + b2 * colors[3 * (long long)v2 + 1];
                c2 = b0 * colors[3 * (long long)v0 + 2] + b1 * colors[3 * (long long)v1 + 2] + b2 * colors[3 * (long long)v2 + 2];
            }
        }
    }
    owner[t] = f;
    texture[3 * t] = c0;
    texture[3 * t + 1] = c1;
    texture[3 * t + 2] = c2;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Per-pixel texels and bilinear weights.  beta_k = w_k / (w_0 + w_1 + w_2) is the perspective-correct barycentric of the pixel centre (w_k =
// b_k / zv_k of pixel_weights), so no depth enters.  The sample is kept inside the chart's box, and the lower tap below the box's last texel:
// every index written lies inside the chart's cell.
__global__ void __launch_bounds__(NT) tex_pixel_texels_kernel(Atlas a, const int32_t* __restrict__ face_id, const float* __restrict__ pix_w, long long HW,
                                                              int32_t* __restrict__ pix_tex, float* __restrict__ pix_tw) {
    const long long pix = (long long)blockIdx.x * NT + threadIdx.x;
    if (pix >= HW) return;
    int t0 = -1, t1 = -1, t2 = -1, t3 = -1;
    float q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
    const int f = face_id[pix];
    const float w0 = pix_w[3 * pix], w1 = pix_w[3 * pix + 1], w2 = pix_w[3 * pix + 2];
    const float sum = w0 + w1 + w2;
    if (f >= 0 && f < a.F && sum > 0.f) {                           // (sum > 0 on every pixel the forward drew; false on NaN)
        const Chart ch = chart_of(a, f);
        // sum beta_k corner_k = corner_0 + beta_1 (corner_1 - corner_0) + beta_2 (corner_2 - corner_0), relative to the cell's origin: the
        // fp32 steps are then those of a coordinate below S, not below R
        const float L = (float)(a.S - 3), far = (float)(a.S - 1);
        // dv is kept under L - du as the bake keeps b2 under 1 - b1: beta_1 + beta_2 <= 1, and with the sum rounded the other way the
        // diagonal tap of half 0 would fall on half 1's first texel with a weight of rounding size
        const float du = fminf(fmaxf(w1 / sum * L, 0.f), L), dv = fminf(fmaxf(w2 / sum * L, 0.f), L - du);
        const float u = ch.half ? far - du : du, v = ch.half ? far - dv : dv;             // inside [lo, hi] by the clamps
        const int i0 = min((int)floorf(u), ch.hi - 1), j0 = min((int)floorf(v), ch.hi - 1);
        const float fu = u - (float)i0, fv = v - (float)j0;
        t0 = (ch.y0 + j0) * a.R + ch.x0 + i0;
        t1 = t0 + 1;
        t2 = t0 + a.R;
        t3 = t2 + 1;
        q0 = (1.f - fu) * (1.f - fv);
        q1 = fu * (1.f - fv);
        q2 = (1.f - fu) * fv;
        q3 = fu * fv;
    }
    pix_tex[4 * pix] = t0;
    pix_tex[4 * pix + 1] = t1;
    pix_tex[4 * pix + 2] = t2;
    pix_tex[4 * pix + 3] = t3;
    pix_tw[4 * pix] = q0;
    pix_tw[4 * pix + 1] = q1;
    pix_tw[4 * pix + 2] = q2;
    pix_tw[4 * pix + 3] = q3;
}

__global__ void __launch_bounds__(NT) tex_shade_kernel(const int32_t* __restrict__ pix_tex, const float* __restrict__ pix_tw, const float* __restrict__ tex,
                                                       int nt, long long HW, float bg0, float bg1, float bg2, float* __restrict__ image) {
    const long long pix = (long long)blockIdx.x * NT + threadIdx.x;
    if (pix >= HW) return;
    const int t0 = pix_tex[4 * pix], t1 = pix_tex[4 * pix + 1], t2 = pix_tex[4 * pix + 2], t3 = pix_tex[4 * pix + 3];
    float c0 = bg0, c1 = bg1, c2 = bg2;
    if (t0 >= 0 && t0 < nt && t1 >= 0 && t1 < nt && t2 >= 0 && t2 < nt && t3 >= 0 && t3 < nt) {
        const float q0 = pix_tw[4 * pix], q1 = pix_tw[4 * pix + 1], q2 = pix_tw[4 * pix + 2], q3 = pix_tw[4 * pix + 3];
        const float *a = tex + 3 * (long long)t0, *b = tex + 3 * (long long)t1, *c = tex + 3 * (long long)t2, *d = tex + 3 * (long long)t3;
        c0 = q0 * a[0] + q1 * b[0] + q2 * c[0] + q3 * d[0];
        c1 = q0 * a[1] + q1 * b[1] + q2 * c[1] + q3 * d[1];
        c2 = q0 * a[2] + q1 * b[2] + q2 * c[2] + q3 * d[2];
    }
    image[pix] = c0;
    image[HW + pix] = c1;
    image[2 * HW + pix] = c2;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The transposed lists.  Four records per covered pixel at rows 4 offsets[pixel] .. + 3, in pixel order: the stable sort on the texel then
// leaves every texel's records in ascending 4 pixel + j.
__global__ void __launch_bounds__(NT) tex_texel_records_kernel(const int32_t* __restrict__ pix_tex, const int32_t* __restrict__ offsets, long long HW, int n,
                                                               unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
    const long long pix = (long long)blockIdx.x * NT + threadIdx.x;
    if (pix >= HW) return;
    if (pix_tex[4 * pix] < 0) return;
    const long long o = 4 * (long long)offsets[pix];
    if (o < 0 || o + 4 > n) return;                                  // (never, with the offsets of this coverage)
    for (int j = 0; j < 4; ++j) {
        keys[o + j] = (unsigned long long)(uint32_t)pix_tex[4 * pix + j];
        vals[o + j] = (uint32_t)(4 * pix + j);
    }
}

// The transpose.  One thread per texel: texels are denser than pixels on the documented path, so most lists are empty and the rest a few
// entries long; a 64-lane wave per row (v3d_recon_mesh_shade_bwd) would idle 63 lanes on them.  Front to back, in list order.
__global__ void __launch_bounds__(NT) tex_shade_bwd_kernel(const int32_t* __restrict__ ranges, const int32_t* __restrict__ ent_pix,
                                                           const float* __restrict__ ent_w, int n, const float* __restrict__ dL_dimage, long long HW,
                                                           long long nt, float* __restrict__ dL_dtex) {
    const long long t = (long long)blockIdx.x * NT + threadIdx.x;
    if (t >= nt) return;
    const int start = max(ranges[2 * t], 0), end = min(ranges[2 * t + 1], n);
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    for (int i = start; i < end; ++i) {
        const long long p = ent_pix[i];
        if (p < 0 || p >= HW) continue;
        const float w = ent_w[i];
        g0 += w * dL_dimage[p];
        g1 += w * dL_dimage[HW + p];
        g2 += w * dL_dimage[2 * HW + p];
    }
    dL_dtex[3 * t] = g0;
    dL_dtex[3 * t + 1] = g1;
    dL_dtex[3 * t + 2] = g2;
}

bool image_ok(int32_t w, int32_t h) { return w > 0 && h > 0 && w <= V3D_RECON_MESH_MAX_IMAGE && h <= V3D_RECON_MESH_MAX_IMAGE; }

// g = ceil(sqrt(ceil(F / 2))), S = floor(R / g); false when a cell would be smaller than 4 texels
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
#define TEX_REQUIRE_IMAGE(name, w, h) \
    RECON_REQUIRE(image_ok(w, h), name ": image %d x %d outside 1 .. %d on a side", (int)(w), (int)(h), V3D_RECON_MESH_MAX_IMAGE)
#define TEX_REQUIRE_ATLAS(name, F, R, a)                                                                                                            \
    RECON_REQUIRE((F) > 0, name ": num_faces must be positive");                                                                                    \
    RECON_REQUIRE((R) >= 1 && (R) <= V3D_RECON_TEX_MAX_SIZE, name ": tex_size %d outside 1 .. %d", (int)(R), V3D_RECON_TEX_MAX_SIZE);              \
    RECON_REQUIRE(atlas_of(F, R, &(a)), name ": texture too small for %d faces: %d x %d leaves cells of %d texels, below %d", (int)(F), (int)(R), \
                  (int)(R), (a).S, V3D_RECON_TEX_MIN_CELL)

extern "C" int v3d_recon_tex_face_uvs(int32_t num_faces, int32_t tex_size, float* vt, v3d_stream_t stream) {
    Atlas a;
    RECON_REQUIRE(vt, "v3d_recon_tex_face_uvs: null argument");
    TEX_REQUIRE_ATLAS("v3d_recon_tex_face_uvs", num_faces, tex_size, a);
    hipLaunchKernelGGL(tex_face_uvs_kernel, dim3(nblk(num_faces)), dim3(NT), 0, ST, a, vt);
    return check_launch("v3d_recon_tex_face_uvs");
}

extern "C" int v3d_recon_tex_bake_vertex_colors(const int32_t* faces, int32_t num_faces, const float* colors, int32_t num_verts, int32_t tex_size,
                                                float fill, int32_t* owner, float* texture, v3d_stream_t stream) {
    Atlas a;
    RECON_REQUIRE(faces && colors && owner && texture, "v3d_recon_tex_bake_vertex_colors: null argument");
    RECON_REQUIRE(num_verts > 0, "v3d_recon_tex_bake_vertex_colors: num_verts must be positive");
    TEX_REQUIRE_ATLAS("v3d_recon_tex_bake_vertex_colors", num_faces, tex_size, a);
    hipLaunchKernelGGL(tex_bake_kernel, dim3(nblk((long long)tex_size * tex_size)), dim3(NT), 0, ST, a, faces, colors, (int)num_verts, fill, owner, texture);
    return check_launch("v3d_recon_tex_bake_vertex_colors");
}

extern "C" int v3d_recon_tex_pixel_texels(const int32_t* face_id, const float* pix_w, int32_t num_faces, int32_t tex_size, int32_t width, int32_t height,
                                          int32_t* pix_tex, float* pix_tw, v3d_stream_t stream) {
    Atlas a;
    RECON_REQUIRE(face_id && pix_w && pix_tex && pix_tw, "v3d_recon_tex_pixel_texels: null argument");
    TEX_REQUIRE_ATLAS("v3d_recon_tex_pixel_texels", num_faces, tex_size, a);
    TEX_REQUIRE_IMAGE("v3d_recon_tex_pixel_texels", width, height);
    const long long HW = (long long)width * height;
    hipLaunchKernelGGL(tex_pixel_texels_kernel, dim3(nblk(HW)), dim3(NT), 0, ST, a, face_id, pix_w, HW, pix_tex, pix_tw);
    return check_launch("v3d_recon_tex_pixel_texels");
}

extern "C" int v3d_recon_tex_shade(const int32_t* pix_tex, const float* pix_tw, const float* texture, int32_t tex_size, int32_t width, int32_t height,
                                   float bg0, float bg1, float bg2, float* image, v3d_stream_t stream) {
    RECON_REQUIRE(pix_tex && pix_tw && texture && image, "v3d_recon_tex_shade: null argument");
    RECON_REQUIRE(tex_size >= 1 && tex_size <= V3D_RECON_TEX_MAX_SIZE, "v3d_recon_tex_shade: tex_size %d outside 1 .. %d", (int)tex_size,
                  V3D_RECON_TEX_MAX_SIZE);
    TEX_REQUIRE_IMAGE("v3d_recon_tex_shade", width, height);
    const long long HW = (long long)width * height;
    hipLaunchKernelGGL(tex_shade_kernel, dim3(nblk(HW)), dim3(NT), 0, ST, pix_tex, pix_tw, texture, (int)(tex_size * tex_size), HW, bg0, bg1, bg2, image);
    return check_launch("v3d_recon_tex_shade");
}

extern "C" int v3d_recon_tex_texel_records(const int32_t* pix_tex, const int32_t* offsets, int32_t width, int32_t height, int32_t num_records,
                                           uint64_t* keys, uint32_t* vals, v3d_stream_t stream) {
    RECON_REQUIRE(pix_tex && offsets && keys && vals, "v3d_recon_tex_texel_records: null argument");
    TEX_REQUIRE_IMAGE("v3d_recon_tex_texel_records", width, height);
    const long long HW = (long long)width * height;
    RECON_REQUIRE(num_records > 0 && num_records % 4 == 0 && num_records <= 4 * HW,
                  "v3d_recon_tex_texel_records: num_records %d is not a positive multiple of 4 up to 4 x the pixel count", (int)num_records);
    hipLaunchKernelGGL(tex_texel_records_kernel, dim3(nblk(HW)), dim3(NT), 0, ST, pix_tex, offsets, HW, (int)num_records, (unsigned long long*)keys, vals);
    return check_launch("v3d_recon_tex_texel_records");
}

extern "C" int v3d_recon_tex_shade_bwd(const int32_t* ranges, const int32_t* ent_pix, const float* ent_w, int32_t num_entries, const float* dL_dimage,
                                       int32_t width, int32_t height, int32_t num_texels, float* dL_dtex, v3d_stream_t stream) {
    RECON_REQUIRE(ranges && dL_dimage && dL_dtex && ((ent_pix && ent_w) || num_entries == 0), "v3d_recon_tex_shade_bwd: null argument");
    RECON_REQUIRE(num_entries >= 0, "v3d_recon_tex_shade_bwd: num_entries must not be negative");
    RECON_REQUIRE(num_texels > 0 && num_texels <= V3D_RECON_TEX_MAX_SIZE * V3D_RECON_TEX_MAX_SIZE,
                  "v3d_recon_tex_shade_bwd: num_texels %d outside 1 .. %d", (int)num_texels, V3D_RECON_TEX_MAX_SIZE * V3D_RECON_TEX_MAX_SIZE);
    TEX_REQUIRE_IMAGE("v3d_recon_tex_shade_bwd", width, height);
    hipLaunchKernelGGL(tex_shade_bwd_kernel, dim3(nblk(num_texels)), dim3(NT), 0, ST, ranges, ent_pix, ent_w, (int)num_entries, dL_dimage,
                       (long long)width * height, (long long)num_texels, dL_dtex);
    return check_launch("v3d_recon_tex_shade_bwd");
}
