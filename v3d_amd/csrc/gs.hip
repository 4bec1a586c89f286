// 3-D Gaussian splatting rasterizer (forward + backward), the exact kNN of the initial scales and the fused D-SSIM + L1 loss of the
// reconstruction step (v3d_amd/recon/, include/v3d_hip.h "Gaussian-splat reconstruction").  Semantics are the published 3DGS rasterizer
// (Kerbl et al. 2023): EWA projection with the 0.3 low-pass, 1.3 tan(fov/2) frustum guard in the Jacobian, cull at view z <= 0.2, 3-sigma
// radius on 16 x 16 tiles, alpha = min(0.99, o exp(power)) skipped for power > 0 or alpha < 1/255, stop below T = 1e-4, background blended
// with the final T, SH degree 0 colour max(0, 0.5 + C0 dc).
//
// Determinism: no atomics of any kind.  Every pixel blends in sorted order; the backward pass writes each sorted instance's gradient, reduced
// over its tile's pixels in a fixed butterfly + wave order, to that instance's own slot, and reduce_instance_grads sums a Gaussian's slots in
// instance order.  The key sort is a stable LSD radix sort whose ranks come from wave ballots (no histogram atomics).
// Built without -ffast-math (v3d_amd/build.py FILE_FLAGS): the tests hold the fp32 forward to an fp64 restatement at 1e-4.
#include "common.h"

namespace {

constexpr int TILE = 16;
constexpr int NT = 256;            // threads per block everywhere (4 waves)
constexpr float SH_C0 = 0.28209479177387814f;

inline unsigned nblk(long long n, int per = NT) { return (unsigned)((n + per - 1) / per); }

__device__ __forceinline__ void quat_rot(const float* q, float R[3][3]) {
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    R[0][0] = 1.f - 2.f * (y * y + z * z); R[0][1] = 2.f * (x * y - r * z); R[0][2] = 2.f * (x * z + r * y);
    R[1][0] = 2.f * (x * y + r * z); R[1][1] = 1.f - 2.f * (x * x + z * z); R[1][2] = 2.f * (y * z - r * x);
    R[2][0] = 2.f * (x * z - r * y); R[2][1] = 2.f * (y * z + r * x); R[2][2] = 1.f - 2.f * (x * x + y * y);
}

// tile rectangle [x0, x1) x [y0, y1) of a Gaussian at pixel (px, py) with radius rad (C casts truncate toward zero, as in the published code)
__device__ __forceinline__ void tile_rect(float px, float py, int rad, int gx, int gy, int& x0, int& y0, int& x1, int& y1) {
    x0 = min(gx, max(0, (int)((px - rad) / TILE)));
    y0 = min(gy, max(0, (int)((py - rad) / TILE)));
    x1 = min(gx, max(0, (int)((px + rad + TILE - 1) / TILE)));
    y1 = min(gy, max(0, (int)((py + rad + TILE - 1) / TILE)));
}

// the one alpha evaluation both render passes share (identical code -> identical skip decisions)
__device__ __forceinline__ float splat_alpha(float2 xy, float4 co, float pxf, float pyf, float& G, float& dx, float& dy, bool& skip) {
    dx = xy.x - pxf;
    dy = xy.y - pyf;
    const float power = -0.5f * (co.x * dx * dx + co.z * dy * dy) - co.y * dx * dy;
    G = expf(power);
    const float alpha = fminf(0.99f, co.w * G);
    skip = power > 0.f || alpha < 1.f / 255.f;
    return alpha;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// kNN: mean squared distance to the 3 nearest other points, exact (brute force over LDS tiles)
__global__ void knn3_kernel(const float* __restrict__ xyz, long long n, float* __restrict__ out) {
    __shared__ float sx[NT], sy[NT], sz[NT];
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    const bool valid = i < n;
    const float qx = valid ? xyz[3 * i] : 0.f, qy = valid ? xyz[3 * i + 1] : 0.f, qz = valid ? xyz[3 * i + 2] : 0.f;
    float b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;
    for (long long base = 0; base < n; base += NT) {
        const long long j = base + threadIdx.x;
        if (j < n) { sx[threadIdx.x] = xyz[3 * j]; sy[threadIdx.x] = xyz[3 * j + 1]; sz[threadIdx.x] = xyz[3 * j + 2]; }
        __syncthreads();
        const int lim = (int)min((long long)NT, n - base);
        for (int k = 0; k < lim; ++k) {
            const float dx = sx[k] - qx, dy = sy[k] - qy, dz = sz[k] - qz;
            const float d = dx * dx + dy * dy + dz * dz;
            if (d < b2 && base + k != i) {
                if (d < b1) {
                    b2 = b1;
                    if (d < b0) { b1 = b0; b0 = d; } else b1 = d;
                } else b2 = d;
            }
        }
        __syncthreads();
    }
    if (valid) out[i] = (b0 + b1 + b2) / 3.f;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// preprocess
__global__ void preprocess_fwd_kernel(long long P, const float* __restrict__ xyz, const float* __restrict__ sraw, const float* __restrict__ rraw,
                                      const float* __restrict__ oraw, const float* __restrict__ fdc, v3d_gs_camera cam, int gx, int gy,
                                      float* __restrict__ means2d, float* __restrict__ conic_op, float* __restrict__ rgb, float* __restrict__ depth,
                                      int32_t* __restrict__ radii, int32_t* __restrict__ tiles, int32_t* __restrict__ clamped) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= P) return;
    radii[i] = 0;
    tiles[i] = 0;
    clamped[i] = 0;
    means2d[2 * i] = 0.f; means2d[2 * i + 1] = 0.f;
    for (int k = 0; k < 4; ++k) conic_op[4 * i + k] = 0.f;
    for (int k = 0; k < 3; ++k) rgb[3 * i + k] = 0.f;
    const float* V = cam.view;
    const float* Pm = cam.proj;
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const float tx = V[0] * x + V[4] * y + V[8] * z + V[12];
    const float ty = V[1] * x + V[5] * y + V[9] * z + V[13];
    const float tz = V[2] * x + V[6] * y + V[10] * z + V[14];
    depth[i] = tz;
    if (tz <= 0.2f) return;
    const float hx = Pm[0] * x + Pm[4] * y + Pm[8] * z + Pm[12];
    const float hy = Pm[1] * x + Pm[5] * y + Pm[9] * z + Pm[13];
    const float hw = Pm[3] * x + Pm[7] * y + Pm[11] * z + Pm[15];
    const float pw = 1.f / (hw + 1e-7f);
    // 3-D covariance R diag(s^2) R^T
    float s[3], q[4], R[3][3];
    for (int k = 0; k < 3; ++k) s[k] = expf(sraw[3 * i + k]);
    float qn = 0.f;
    for (int k = 0; k < 4; ++k) { q[k] = rraw[4 * i + k]; qn += q[k] * q[k]; }
    qn = 1.f / sqrtf(qn);
    for (int k = 0; k < 4; ++k) q[k] *= qn;
    quat_rot(q, R);
    float Sg[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) Sg[a][b] = R[a][0] * s[0] * s[0] * R[b][0] + R[a][1] * s[1] * s[1] * R[b][1] + R[a][2] * s[2] * s[2] * R[b][2];
    // EWA: T = J W, cov2 = T Sg T^T
    const float W = (float)cam.width, H = (float)cam.height;
    const float fx = W / (2.f * cam.tanfovx), fy = H / (2.f * cam.tanfovy);
    const float limx = 1.3f * cam.tanfovx, limy = 1.3f * cam.tanfovy;
    const float txc = fminf(limx, fmaxf(-limx, tx / tz)) * tz, tyc = fminf(limy, fmaxf(-limy, ty / tz)) * tz;
    const float J00 = fx / tz, J02 = -fx * txc / (tz * tz), J11 = fy / tz, J12 = -fy * tyc / (tz * tz);
    float Tm[2][3];
    for (int c = 0; c < 3; ++c) {   // W[r][c] = V[4c + r]
        Tm[0][c] = J00 * V[4 * c + 0] + J02 * V[4 * c + 2];
        Tm[1][c] = J11 * V[4 * c + 1] + J12 * V[4 * c + 2];
    }
    float TS[2][3];
    for (int r = 0; r < 2; ++r)
        for (int c = 0; c < 3; ++c) TS[r][c] = Tm[r][0] * Sg[0][c] + Tm[r][1] * Sg[1][c] + Tm[r][2] * Sg[2][c];
    const float a = TS[0][0] * Tm[0][0] + TS[0][1] * Tm[0][1] + TS[0][2] * Tm[0][2] + 0.3f;
    const float b = TS[0][0] * Tm[1][0] + TS[0][1] * Tm[1][1] + TS[0][2] * Tm[1][2];
    const float c = TS[1][0] * Tm[1][0] + TS[1][1] * Tm[1][1] + TS[1][2] * Tm[1][2] + 0.3f;
    const float det = a * c - b * b;
    if (det == 0.f) return;
    const float di = 1.f / det;
    const float mid = 0.5f * (a + c);
    const float l1 = mid + sqrtf(fmaxf(0.1f, mid * mid - det)), l2 = mid - sqrtf(fmaxf(0.1f, mid * mid - det));
    const int rad = (int)ceilf(3.f * sqrtf(fmaxf(l1, l2)));
    const float px = ((hx * pw + 1.f) * W - 1.f) * 0.5f, py = ((hy * pw + 1.f) * H - 1.f) * 0.5f;
    int x0, y0, x1, y1;
    tile_rect(px, py, rad, gx, gy, x0, y0, x1, y1);
    const int area = (x1 - x0) * (y1 - y0);
    if (area == 0) return;
    int cl = 0;
    for (int k = 0; k < 3; ++k) {
        const float v = SH_C0 * fdc[3 * i + k] + 0.5f;
        if (v < 0.f) cl |= 1 << k;
        rgb[3 * i + k] = fmaxf(v, 0.f);
    }
    clamped[i] = cl;
    means2d[2 * i] = px;
    means2d[2 * i + 1] = py;
    conic_op[4 * i] = c * di;
    conic_op[4 * i + 1] = -b * di;
    conic_op[4 * i + 2] = a * di;
    conic_op[4 * i + 3] = 1.f / (1.f + expf(-oraw[i]));
    radii[i] = rad;
    tiles[i] = area;
}

// g9 per Gaussian: dL/d(pixel x, pixel y), dL/d(conic A, B, C) with power = -0.5 (A dx^2 + C dy^2) - B dx dy, dL/d(opacity), dL/d(rgb)
__global__ void preprocess_bwd_kernel(long long P, const float* __restrict__ xyz, const float* __restrict__ sraw, const float* __restrict__ rraw,
                                      const float* __restrict__ oraw, v3d_gs_camera cam, const int32_t* __restrict__ radii,
                                      const int32_t* __restrict__ clamped, const float* __restrict__ g9, float* __restrict__ d_xyz,
                                      float* __restrict__ d_s, float* __restrict__ d_r, float* __restrict__ d_o, float* __restrict__ d_fdc,
                                      float* __restrict__ d_m2) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= P) return;
    for (int k = 0; k < 3; ++k) { d_xyz[3 * i + k] = 0.f; d_s[3 * i + k] = 0.f; d_fdc[3 * i + k] = 0.f; }
    for (int k = 0; k < 4; ++k) d_r[4 * i + k] = 0.f;
    d_o[i] = 0.f;
    d_m2[2 * i] = 0.f; d_m2[2 * i + 1] = 0.f;
    if (radii[i] <= 0) return;
    const float* g = g9 + 9 * i;
    const float* V = cam.view;
    const float* Pm = cam.proj;
    const float W = (float)cam.width, H = (float)cam.height;
    // colour and opacity
    const int cl = clamped[i];
    for (int k = 0; k < 3; ++k) d_fdc[3 * i + k] = (cl >> k) & 1 ? 0.f : SH_C0 * g[6 + k];
    const float o = 1.f / (1.f + expf(-oraw[i]));
    d_o[i] = g[5] * o * (1.f - o);
    // screen-space mean (NDC) -> world position through the projection
    const float dnx = g[0] * 0.5f * W, dny = g[1] * 0.5f * H;
    d_m2[2 * i] = dnx;
    d_m2[2 * i + 1] = dny;
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const float hx = Pm[0] * x + Pm[4] * y + Pm[8] * z + Pm[12];
    const float hy = Pm[1] * x + Pm[5] * y + Pm[9] * z + Pm[13];
    const float hw = Pm[3] * x + Pm[7] * y + Pm[11] * z + Pm[15];
    const float pw = 1.f / (hw + 1e-7f);
    float dp[3];
    for (int k = 0; k < 3; ++k)
        dp[k] = dnx * (Pm[4 * k] * pw - hx * pw * pw * Pm[4 * k + 3]) + dny * (Pm[4 * k + 1] * pw - hy * pw * pw * Pm[4 * k + 3]);
    // recompute the forward quantities of the covariance path
    const float tx = V[0] * x + V[4] * y + V[8] * z + V[12];
    const float ty = V[1] * x + V[5] * y + V[9] * z + V[13];
    const float tz = V[2] * x + V[6] * y + V[10] * z + V[14];
    float s[3], q[4], R[3][3];
    for (int k = 0; k < 3; ++k) s[k] = expf(sraw[3 * i + k]);
    float qn2 = 0.f;
    for (int k = 0; k < 4; ++k) { q[k] = rraw[4 * i + k]; qn2 += q[k] * q[k]; }
    const float qinv = 1.f / sqrtf(qn2);
    for (int k = 0; k < 4; ++k) q[k] *= qinv;
    quat_rot(q, R);
    float Sg[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) Sg[a][b] = R[a][0] * s[0] * s[0] * R[b][0] + R[a][1] * s[1] * s[1] * R[b][1] + R[a][2] * s[2] * s[2] * R[b][2];
    const float fx = W / (2.f * cam.tanfovx), fy = H / (2.f * cam.tanfovy);
    const float limx = 1.3f * cam.tanfovx, limy = 1.3f * cam.tanfovy;
    const float txtz = tx / tz, tytz = ty / tz;
    const float xg = (txtz < -limx || txtz > limx) ? 0.f : 1.f, yg = (tytz < -limy || tytz > limy) ? 0.f : 1.f;
    const float txc = fminf(limx, fmaxf(-limx, txtz)) * tz, tyc = fminf(limy, fmaxf(-limy, tytz)) * tz;
    const float J00 = fx / tz, J02 = -fx * txc / (tz * tz), J11 = fy / tz, J12 = -fy * tyc / (tz * tz);
    float Wm[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Wm[r][c] = V[4 * c + r];
    float Tm[2][3];
    for (int c = 0; c < 3; ++c) { Tm[0][c] = J00 * Wm[0][c] + J02 * Wm[2][c]; Tm[1][c] = J11 * Wm[1][c] + J12 * Wm[2][c]; }
    float TS[2][3];
    for (int r = 0; r < 2; ++r)
        for (int c = 0; c < 3; ++c) TS[r][c] = Tm[r][0] * Sg[0][c] + Tm[r][1] * Sg[1][c] + Tm[r][2] * Sg[2][c];
    const float a = TS[0][0] * Tm[0][0] + TS[0][1] * Tm[0][1] + TS[0][2] * Tm[0][2] + 0.3f;
    const float b = TS[0][0] * Tm[1][0] + TS[0][1] * Tm[1][1] + TS[0][2] * Tm[1][2];
    const float c = TS[1][0] * Tm[1][0] + TS[1][1] * Tm[1][1] + TS[1][2] * Tm[1][2] + 0.3f;
    const float det = a * c - b * b;
    const float d2 = 1.f / (det * det);
    const float gA = g[2], gB = g[3], gC = g[4];
    const float da = (-c * c * gA + b * c * gB - b * b * gC) * d2;
    const float db = (2.f * b * c * gA - (det + 2.f * b * b) * gB + 2.f * a * b * gC) * d2;
    const float dc = (-b * b * gA + a * b * gB - a * a * gC) * d2;
    const float Gc[2][2] = {{da, 0.5f * db}, {0.5f * db, dc}};
    // dL/dSigma = T^T Gc T ; dL/dT = 2 Gc T Sigma
    float GT[2][3];
    for (int r = 0; r < 2; ++r)
        for (int cc = 0; cc < 3; ++cc) GT[r][cc] = Gc[r][0] * Tm[0][cc] + Gc[r][1] * Tm[1][cc];
    float dS[3][3];
    for (int r = 0; r < 3; ++r)
        for (int cc = 0; cc < 3; ++cc) dS[r][cc] = Tm[0][r] * GT[0][cc] + Tm[1][r] * GT[1][cc];
    float dT[2][3];
    for (int r = 0; r < 2; ++r)
        for (int cc = 0; cc < 3; ++cc) dT[r][cc] = 2.f * (GT[r][0] * Sg[0][cc] + GT[r][1] * Sg[1][cc] + GT[r][2] * Sg[2][cc]);
    // dL/dJ = dT W^T (only the four non-zero entries of J matter)
    const float dJ00 = dT[0][0] * Wm[0][0] + dT[0][1] * Wm[0][1] + dT[0][2] * Wm[0][2];
    const float dJ02 = dT[0][0] * Wm[2][0] + dT[0][1] * Wm[2][1] + dT[0][2] * Wm[2][2];
    const float dJ11 = dT[1][0] * Wm[1][0] + dT[1][1] * Wm[1][1] + dT[1][2] * Wm[1][2];
    const float dJ12 = dT[1][0] * Wm[2][0] + dT[1][1] * Wm[2][1] + dT[1][2] * Wm[2][2];
    const float tz2 = 1.f / (tz * tz), tz3 = tz2 / tz;
    const float dtx = xg * -fx * tz2 * dJ02, dty = yg * -fy * tz2 * dJ12;
    const float dtz = -fx * tz2 * dJ00 - fy * tz2 * dJ11 + 2.f * fx * txc * tz3 * dJ02 + 2.f * fy * tyc * tz3 * dJ12;
    for (int k = 0; k < 3; ++k) dp[k] += Wm[0][k] * dtx + Wm[1][k] * dty + Wm[2][k] * dtz;
    for (int k = 0; k < 3; ++k) d_xyz[3 * i + k] = dp[k];
    // Sigma = M M^T, M = R diag(s): dM = 2 dS M
    float dR[3][3];
    float ds[3] = {0.f, 0.f, 0.f};
    for (int r = 0; r < 3; ++r)
        for (int j = 0; j < 3; ++j) {
            const float dM = 2.f * (dS[r][0] * R[0][j] + dS[r][1] * R[1][j] + dS[r][2] * R[2][j]) * s[j];
            ds[j] += dM * R[r][j];
            dR[r][j] = dM * s[j];
        }
    for (int k = 0; k < 3; ++k) d_s[3 * i + k] = ds[k] * s[k];
    const float qr = q[0], qx = q[1], qy = q[2], qz = q[3];
    float dq[4];
    dq[0] = 2.f * (-qz * dR[0][1] + qy * dR[0][2] + qz * dR[1][0] - qx * dR[1][2] - qy * dR[2][0] + qx * dR[2][1]);
    dq[1] = 2.f * (qy * dR[0][1] + qz * dR[0][2] + qy * dR[1][0] - 2.f * qx * dR[1][1] - qr * dR[1][2] + qz * dR[2][0] + qr * dR[2][1] - 2.f * qx * dR[2][2]);
    dq[2] = 2.f * (-2.f * qy * dR[0][0] + qx * dR[0][1] + qr * dR[0][2] + qx * dR[1][0] + qz * dR[1][2] - qr * dR[2][0] + qz * dR[2][1] - 2.f * qy * dR[2][2]);
    dq[3] = 2.f * (-2.f * qz * dR[0][0] - qr * dR[0][1] + qx * dR[0][2] + qr * dR[1][0] - 2.f * qz * dR[1][1] + qy * dR[1][2] + qx * dR[2][0] + qy * dR[2][1]);
    const float qd = q[0] * dq[0] + q[1] * dq[1] + q[2] * dq[2] + q[3] * dq[3];
    for (int k = 0; k < 4; ++k) d_r[4 * i + k] = (dq[k] - q[k] * qd) * qinv;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// exclusive int32 scan: block sums -> scan of the block sums (one block) -> per-block scan with offset.  out[n] = total.
constexpr int SCAN_ITEMS = 16, SCAN_CHUNK = NT * SCAN_ITEMS;

__device__ __forceinline__ int block_excl_scan(int v, int* sh, int& total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < NT; o <<= 1) {
        const int add = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const int incl = sh[t];
    total = sh[NT - 1];
    __syncthreads();
    return incl - v;
}

__global__ void scan_sums_kernel(const int32_t* __restrict__ in, long long n, int32_t* __restrict__ bsum) {
    __shared__ int sh[NT];
    const long long base = (long long)blockIdx.x * SCAN_CHUNK + (long long)threadIdx.x * SCAN_ITEMS;
    int s = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) s += base + k < n ? in[base + k] : 0;
    int total;
    block_excl_scan(s, sh, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ void scan_top_kernel(int32_t* __restrict__ bsum, long long nb, int32_t* __restrict__ out_total) {
    __shared__ int sh[NT];
    int carry = 0;
    for (long long base = 0; base < nb; base += NT) {
        const long long j = base + threadIdx.x;
        const int v = j < nb ? bsum[j] : 0;
        int total;
        const int ex = block_excl_scan(v, sh, total);
        if (j < nb) bsum[j] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *out_total = carry;
}

__global__ void scan_apply_kernel(const int32_t* __restrict__ in, long long n, const int32_t* __restrict__ bsum, int32_t* __restrict__ out) {
    __shared__ int sh[NT];
    const long long base = (long long)blockIdx.x * SCAN_CHUNK + (long long)threadIdx.x * SCAN_ITEMS;
    int v[SCAN_ITEMS];
    int s = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) { v[k] = base + k < n ? in[base + k] : 0; s += v[k]; }
    int total;
    int run = block_excl_scan(s, sh, total) + bsum[blockIdx.x];
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// stable LSD radix sort, 8-bit digits.  A block owns RS_SUB consecutive sub-tiles of 256 keys; inside a sub-tile a key's rank among equal
// digits of its wave comes from 8 ballots, the waves are ordered through LDS, and a per-digit running offset carries across sub-tiles.
constexpr int RS_BITS = 8, RS_DIG = 1 << RS_BITS, RS_SUB = 16, RS_CHUNK = NT * RS_SUB;
static_assert(NT == RS_DIG, "the radix kernels give thread t digit t (counts, running offsets)");

__device__ __forceinline__ unsigned long long peers_of(unsigned d, bool valid) {
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < RS_BITS; ++b) {
        const unsigned long long m = __ballot((d >> b) & 1u);
        peers &= ((d >> b) & 1u) ? m : ~m;
    }
    return peers;
}

__global__ void radix_count_kernel(const uint64_t* __restrict__ keys, long long n, int shift, unsigned dmask, long long nb,
                                   int32_t* __restrict__ counts) {
    __shared__ int whist[NT / V3D_WAVE][RS_DIG];
    const int t = threadIdx.x, w = t / V3D_WAVE, lane = t % V3D_WAVE;
    for (int k = t; k < (NT / V3D_WAVE) * RS_DIG; k += NT) (&whist[0][0])[k] = 0;
    __syncthreads();
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int sub = 0; sub < RS_SUB; ++sub) {
        const long long j = (long long)blockIdx.x * RS_CHUNK + sub * NT + t;
        const bool valid = j < n;
        const unsigned d = valid ? (unsigned)(keys[j] >> shift) & dmask : 0u;
        const unsigned long long peers = peers_of(d, valid);
        if (valid && (peers & lt) == 0) whist[w][d] += __popcll(peers);      // one leader lane per digit and wave
    }
    __syncthreads();
    int s = 0;
    for (int ww = 0; ww < NT / V3D_WAVE; ++ww) s += whist[ww][t];
    counts[(long long)t * nb + blockIdx.x] = s;        // digit-major: the exclusive scan gives stable global offsets
}

__global__ void radix_scatter_kernel(const uint64_t* __restrict__ kin, const uint32_t* __restrict__ vin, long long n, int shift, unsigned dmask,
                                     long long nb, const int32_t* __restrict__ offs, uint64_t* __restrict__ kout, uint32_t* __restrict__ vout) {
    __shared__ int whist[NT / V3D_WAVE][RS_DIG];
    __shared__ int run[RS_DIG];
    const int t = threadIdx.x, w = t / V3D_WAVE, lane = t % V3D_WAVE;
    run[t] = offs[(long long)t * nb + blockIdx.x];
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int sub = 0; sub < RS_SUB; ++sub) {
        for (int k = t; k < (NT / V3D_WAVE) * RS_DIG; k += NT) (&whist[0][0])[k] = 0;
        __syncthreads();
        const long long j = (long long)blockIdx.x * RS_CHUNK + sub * NT + t;
        const bool valid = j < n;
        const uint64_t key = valid ? kin[j] : 0ull;
        const uint32_t val = valid ? vin[j] : 0u;
        const unsigned d = (unsigned)(key >> shift) & dmask;
        const unsigned long long peers = peers_of(d, valid);
        const int rank = __popcll(peers & lt);
        if (valid && rank == 0) whist[w][d] = __popcll(peers);
        __syncthreads();
        {   // thread t owns digit t: wave offsets in wave order, then advance the running offset
            int o = run[t];
            for (int ww = 0; ww < NT / V3D_WAVE; ++ww) { const int c = whist[ww][t]; whist[ww][t] = o; o += c; }
            run[t] = o;
        }
        __syncthreads();
        if (valid) {
            const long long pos = (long long)whist[w][d] + rank;
            kout[pos] = key;
            vout[pos] = val;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
__global__ void duplicate_keys_kernel(long long P, const float* __restrict__ means2d, const int32_t* __restrict__ radii, const float* __restrict__ depth,
                                      const int32_t* __restrict__ offsets, int gx, int gy, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const long long g = (long long)blockIdx.x * NT + threadIdx.x;
    if (g >= P || radii[g] <= 0) return;
    int x0, y0, x1, y1;
    tile_rect(means2d[2 * g], means2d[2 * g + 1], radii[g], gx, gy, x0, y0, x1, y1);
    long long off = offsets[g];
    const long long end = offsets[g + 1];
    const uint64_t dbits = (uint64_t)__float_as_uint(depth[g]);
    for (int ty = y0; ty < y1; ++ty)
        for (int tx = x0; tx < x1; ++tx) {
            if (off >= end) return;
            keys[off] = ((uint64_t)(ty * gx + tx) << 32) | dbits;
            vals[off] = (uint32_t)g;
            ++off;
        }
}

// ranges[tile] = [start, end) in the sorted list; inst_pos[u] = sorted position of unsorted instance u (instance u of Gaussian g is
// offsets[g] + its tile's row-major index inside g's rectangle, exactly as duplicate_keys laid it out)
__global__ void tile_ranges_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, long long n, const float* __restrict__ means2d,
                                   const int32_t* __restrict__ radii, const int32_t* __restrict__ offsets, int gx, int gy,
                                   int32_t* __restrict__ ranges, int32_t* __restrict__ inst_pos) {
    const long long s = (long long)blockIdx.x * NT + threadIdx.x;
    if (s >= n) return;
    const long long ntiles = (long long)gx * gy;
    const unsigned tile = (unsigned)(keys[s] >> 32);
    if (tile >= ntiles) return;
    if (s == 0) ranges[2 * tile] = 0;
    else {
        const unsigned prev = (unsigned)(keys[s - 1] >> 32);
        if (prev != tile) {
            if (prev < ntiles) ranges[2 * prev + 1] = (int32_t)s;
            ranges[2 * tile] = (int32_t)s;
        }
    }
    if (s == n - 1) ranges[2 * tile + 1] = (int32_t)n;
    const uint32_t g = vals[s];
    int x0, y0, x1, y1;
    tile_rect(means2d[2 * g], means2d[2 * g + 1], radii[g], gx, gy, x0, y0, x1, y1);
    const int tx = (int)(tile % gx), ty = (int)(tile / gx);
    const long long u = (long long)offsets[g] + (long long)(ty - y0) * (x1 - x0) + (tx - x0);
    if (u >= 0 && u < n) inst_pos[u] = (int32_t)s;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) render_fwd_kernel(const int32_t* __restrict__ ranges, const uint32_t* __restrict__ gid,
                                                        const float* __restrict__ means2d, const float* __restrict__ conic_op,
                                                        const float* __restrict__ rgb, v3d_gs_camera cam, int gx, float* __restrict__ out,
                                                        float* __restrict__ final_T, int32_t* __restrict__ n_contrib) {
    __shared__ float2 s_xy[NT];
    __shared__ float4 s_co[NT];
    __shared__ float s_c[NT][3];
    const int W = cam.width, H = cam.height;
    const int tile = blockIdx.x, t = threadIdx.x;
    const int px = (tile % gx) * TILE + (t % TILE), py = (tile / gx) * TILE + (t / TILE);
    const bool inside = px < W && py < H;
    const float pxf = (float)px, pyf = (float)py;
    const int start = ranges[2 * tile], end = ranges[2 * tile + 1];
    bool done = !inside;
    float T = 1.f, C[3] = {0.f, 0.f, 0.f};
    int contributor = 0, last = 0;
    int todo = end - start;
    for (int base = start; base < end; base += NT, todo -= NT) {
        if (__syncthreads_count(done) == NT) break;
        if (base + t < end) {
            const uint32_t g = gid[base + t];
            s_xy[t] = make_float2(means2d[2 * g], means2d[2 * g + 1]);
            s_co[t] = make_float4(conic_op[4 * g], conic_op[4 * g + 1], conic_op[4 * g + 2], conic_op[4 * g + 3]);
            s_c[t][0] = rgb[3 * g]; s_c[t][1] = rgb[3 * g + 1]; s_c[t][2] = rgb[3 * g + 2];
        }
        __syncthreads();
        const int cnt = min(NT, todo);
        for (int j = 0; !done && j < cnt; ++j) {
            ++contributor;
            float G, dx, dy;
            bool skip;
            const float alpha = splat_alpha(s_xy[j], s_co[j], pxf, pyf, G, dx, dy, skip);
            if (skip) continue;
            const float tT = T * (1.f - alpha);
            if (tT < 0.0001f) { done = true; continue; }
            for (int ch = 0; ch < 3; ++ch) C[ch] += s_c[j][ch] * alpha * T;
            T = tT;
            last = contributor;
        }
    }
    if (inside) {
        const long long pix = (long long)py * W + px, HW = (long long)H * W;
        for (int ch = 0; ch < 3; ++ch) out[ch * HW + pix] = C[ch] + T * cam.bg[ch];
        final_T[pix] = T;
        n_contrib[pix] = last;
    }
}

constexpr int BWD_BATCH = 64, NG = 9;

__global__ void __launch_bounds__(NT) render_bwd_kernel(const int32_t* __restrict__ ranges, const uint32_t* __restrict__ gid,
                                                        const float* __restrict__ means2d, const float* __restrict__ conic_op,
                                                        const float* __restrict__ rgb, v3d_gs_camera cam, int gx, const float* __restrict__ final_T,
                                                        const int32_t* __restrict__ n_contrib, const float* __restrict__ dimg,
                                                        float* __restrict__ inst_grads) {
    __shared__ float2 s_xy[BWD_BATCH];
    __shared__ float4 s_co[BWD_BATCH];
    __shared__ float s_c[BWD_BATCH][3];
    __shared__ float s_red[BWD_BATCH][NT / V3D_WAVE][NG];
    __shared__ int s_max;
    const int W = cam.width, H = cam.height;
    const int tile = blockIdx.x, t = threadIdx.x, w = t / V3D_WAVE, lane = t % V3D_WAVE;
    const int px = (tile % gx) * TILE + (t % TILE), py = (tile / gx) * TILE + (t / TILE);
    const bool inside = px < W && py < H;
    const float pxf = (float)px, pyf = (float)py;
    const int start = ranges[2 * tile], end = ranges[2 * tile + 1];
    const long long pix = (long long)py * W + px, HW = (long long)H * W;
    const float T_final = inside ? final_T[pix] : 0.f;
    float T = T_final;
    const int last = inside ? n_contrib[pix] : 0;
    float dpix[3], accum[3] = {0.f, 0.f, 0.f}, last_color[3] = {0.f, 0.f, 0.f};
    for (int ch = 0; ch < 3; ++ch) dpix[ch] = inside ? dimg[ch * HW + pix] : 0.f;
    const float bg_dot = cam.bg[0] * dpix[0] + cam.bg[1] * dpix[1] + cam.bg[2] * dpix[2];
    float last_alpha = 0.f;
    // instances at list position >= the largest last contributor of the tile contribute nothing
    if (t == 0) s_max = 0;
    __syncthreads();
    for (int ww = 0; ww < NT / V3D_WAVE; ++ww) {       // block max in wave order (reads are race-free: one writer per step)
        int m = last;
        for (int o = V3D_WAVE / 2; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, V3D_WAVE));
        if (w == ww && lane == 0) s_max = max(s_max, m);
        __syncthreads();
    }
    const int maxlast = s_max;
    const int n = end - start;
    for (int kb1 = n; kb1 > 0; kb1 -= BWD_BATCH) {
        const int kb0 = max(0, kb1 - BWD_BATCH), cnt = kb1 - kb0;
        if (kb0 >= maxlast) {
            for (int e = t; e < cnt * NG; e += NT) inst_grads[(long long)(start + kb0) * NG + e] = 0.f;
            continue;
        }
        if (t < cnt) {
            const uint32_t g = gid[start + kb0 + t];
            s_xy[t] = make_float2(means2d[2 * g], means2d[2 * g + 1]);
            s_co[t] = make_float4(conic_op[4 * g], conic_op[4 * g + 1], conic_op[4 * g + 2], conic_op[4 * g + 3]);
            s_c[t][0] = rgb[3 * g]; s_c[t][1] = rgb[3 * g + 1]; s_c[t][2] = rgb[3 * g + 2];
        }
        __syncthreads();
        for (int jj = cnt - 1; jj >= 0; --jj) {
            const int k = kb0 + jj;     // position in the tile's list, front to back
            float v[NG];
            for (int q = 0; q < NG; ++q) v[q] = 0.f;
            bool contrib = false;
            if (k < last) {
                float G, dx, dy;
                bool skip;
                const float4 co = s_co[jj];
                const float alpha = splat_alpha(s_xy[jj], co, pxf, pyf, G, dx, dy, skip);
                if (!skip) {
                    contrib = true;
                    T = T / (1.f - alpha);
                    const float wgt = alpha * T;
                    float dalpha = 0.f;
                    for (int ch = 0; ch < 3; ++ch) {
                        const float c = s_c[jj][ch];
                        accum[ch] = last_alpha * last_color[ch] + (1.f - last_alpha) * accum[ch];
                        last_color[ch] = c;
                        dalpha += (c - accum[ch]) * dpix[ch];
                        v[6 + ch] = wgt * dpix[ch];
                    }
                    dalpha *= T;
                    last_alpha = alpha;
                    dalpha += (-T_final / (1.f - alpha)) * bg_dot;
                    const float dG = co.w * dalpha;
                    const float dpow = dG * G;
                    v[0] = dpow * (-co.x * dx - co.y * dy);
                    v[1] = dpow * (-co.z * dy - co.y * dx);
                    v[2] = dpow * -0.5f * dx * dx;
                    v[3] = dpow * -dx * dy;
                    v[4] = dpow * -0.5f * dy * dy;
                    v[5] = G * dalpha;
                }
            }
            if (__ballot(contrib)) {
                for (int q = 0; q < NG; ++q)
                    for (int o = V3D_WAVE / 2; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o, V3D_WAVE);
            }
            if (lane == 0)
                for (int q = 0; q < NG; ++q) s_red[jj][w][q] = v[q];
        }
        __syncthreads();
        for (int e = t; e < cnt * NG; e += NT) {
            const int i = e / NG, q = e % NG;
            float s = 0.f;
            for (int ww = 0; ww < NT / V3D_WAVE; ++ww) s += s_red[i][ww][q];
            inst_grads[(long long)(start + kb0 + i) * NG + q] = s;
        }
        __syncthreads();
    }
}

__global__ void reduce_grads_kernel(const float* __restrict__ inst_grads, const int32_t* __restrict__ offsets, const int32_t* __restrict__ inst_pos,
                                    long long P, float* __restrict__ g9) {
    const long long g = (long long)blockIdx.x * NT + threadIdx.x;
    if (g >= P) return;
    float acc[NG];
    for (int q = 0; q < NG; ++q) acc[q] = 0.f;
    for (long long u = offsets[g]; u < offsets[g + 1]; ++u) {
        const long long s = inst_pos[u];
        for (int q = 0; q < NG; ++q) acc[q] += inst_grads[s * NG + q];
    }
    for (int q = 0; q < NG; ++q) g9[g * NG + q] = acc[q];
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// fused D-SSIM + L1.  Window: 11 taps, sigma 1.5, zero padding 5, per channel; the 2-D window is the outer product of the 1-D one.
struct Win { float g[11]; };

// horizontal pass: nmaps source maps built from (x, y) per mode.  The five moment maps of the forward (MODE 0) are accumulated and kept in
// fp64: var = E[x^2] - E[x]^2 cancels to ~0 on flat image regions, and what fp32 moments leave of it (a few 1e-9) is not small beside
// c2 = 9e-4 (a constant image pair was off by 3e-5 in SSIM)
template <int MODE, typename TO>
__global__ void ssim_hblur_kernel(const float* __restrict__ a, const float* __restrict__ b, long long C, int H, int W, Win win,
                                  TO* __restrict__ out) {
    const long long CHW = C * H * W;
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= CHW) return;
    const int x = (int)(i % W);
    constexpr int NM = MODE == 0 ? 5 : 3;
    TO acc[NM];
    for (int m = 0; m < NM; ++m) acc[m] = 0;
    for (int k = 0; k < 11; ++k) {
        const int xx = x + k - 5;
        if (xx < 0 || xx >= W) continue;
        const long long j = i + (k - 5);
        const TO wk = win.g[k];
        if (MODE == 0) {
            const TO u = a[j], v = b[j];
            acc[0] += wk * u; acc[1] += wk * v; acc[2] += wk * (u * u); acc[3] += wk * (v * v); acc[4] += wk * (u * v);
        } else {
            for (int m = 0; m < NM; ++m) acc[m] += wk * a[m * CHW + j];
        }
    }
    for (int m = 0; m < NM; ++m) out[m * CHW + i] = acc[m];
}

__device__ __forceinline__ void block_sum2(float& s0, float& s1, float (*sh)[NT]) {
    const int t = threadIdx.x;
    sh[0][t] = s0; sh[1][t] = s1;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (t < o) { sh[0][t] += sh[0][t + o]; sh[1][t] += sh[1][t + o]; }
        __syncthreads();
    }
    s0 = sh[0][0]; s1 = sh[1][0];
}

// vertical pass + SSIM map; stores dS/dmu1, dS/dE[x^2], dS/dE[xy] per pixel and per-block partial sums (S, |x - y|)
__global__ void ssim_vfwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const double* __restrict__ h5, long long C, int H, int W,
                                 Win win, float* __restrict__ gmaps, float* __restrict__ partial) {
    __shared__ float sh[2][NT];
    const long long CHW = C * H * W;
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    float S = 0.f, l1 = 0.f;
    if (i < CHW) {
        const int yy = (int)((i / W) % H);
        double m[5] = {0., 0., 0., 0., 0.};
        for (int k = 0; k < 11; ++k) {
            const int r = yy + k - 5;
            if (r < 0 || r >= H) continue;
            const long long j = i + (long long)(k - 5) * W;
            for (int q = 0; q < 5; ++q) m[q] += (double)win.g[k] * h5[q * CHW + j];
        }
        const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
        const double mu1 = m[0], mu2 = m[1];
        const double s11 = m[2] - mu1 * mu1, s22 = m[3] - mu2 * mu2, s12 = m[4] - mu1 * mu2;
        const double A1 = 2. * mu1 * mu2 + C1, A2 = 2. * s12 + C2, B1 = mu1 * mu1 + mu2 * mu2 + C1, B2 = s11 + s22 + C2;
        const double inv = 1. / (B1 * B2);
        const double Sd = A1 * A2 * inv;
        S = (float)Sd;
        gmaps[i] = (float)((2. * mu2 * A2 - 2. * mu2 * A1) * inv - Sd * (2. * mu1 / B1 - 2. * mu1 / B2));
        gmaps[CHW + i] = (float)(-Sd / B2);
        gmaps[2 * CHW + i] = (float)(2. * A1 * inv);
        l1 = fabsf(x[i] - y[i]);
    }
    block_sum2(S, l1, sh);
    if (threadIdx.x == 0) { partial[2 * blockIdx.x] = S; partial[2 * blockIdx.x + 1] = l1; }
}

__global__ void ssim_final_kernel(const float* __restrict__ partial, long long nb, long long N, float lambda, float* __restrict__ out3) {
    __shared__ float sh[2][NT];
    float S = 0.f, l1 = 0.f;
    for (long long b = threadIdx.x; b < nb; b += NT) { S += partial[2 * b]; l1 += partial[2 * b + 1]; }
    block_sum2(S, l1, sh);
    if (threadIdx.x == 0) {
        const float ssim = S / (float)N, L1 = l1 / (float)N;
        out3[0] = (1.f - lambda) * L1 + lambda * (1.f - ssim);
        out3[1] = ssim;
        out3[2] = L1;
    }
}

__global__ void ssim_vbwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ h3, long long C, int H, int W,
                                 Win win, float lambda, const float* __restrict__ dloss, float* __restrict__ grad) {
    const long long CHW = C * H * W;
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= CHW) return;
    const int yy = (int)((i / W) % H);
    float m[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 11; ++k) {
        const int r = yy + k - 5;
        if (r < 0 || r >= H) continue;
        const long long j = i + (long long)(k - 5) * W;
        for (int q = 0; q < 3; ++q) m[q] += win.g[k] * h3[q * CHW + j];
    }
    const float u = x[i], v = y[i], invN = 1.f / (float)CHW;
    const float dS = m[0] + 2.f * u * m[1] + v * m[2];
    const float d = u - v;
    const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    grad[i] = dloss[0] * invN * (-lambda * dS + (1.f - lambda) * sgn);
}

Win ssim_window() {
    float gf[11];
    double sd = 0.;
    for (int k = 0; k < 11; ++k) gf[k] = (float)exp(-0.5 * ((k - 5) / 1.5) * ((k - 5) / 1.5));
    for (int k = 0; k < 11; ++k) sd += gf[k];
    // fp32 normalisation, as the published loss builds its window.  The fp32 sum of the taps is the correctly rounded one (what a
    // pairwise / vectorised fp32 sum of these 11 numbers gives; adding them left to right in fp32 lands one ulp below it, and a window
    // whose sum is off by 7e-8 moves the variance of a flat region, c^2 S (1 - S), by ~1e-8 beside c2 = 9e-4)
    const float sf = (float)sd;
    Win w;
    for (int k = 0; k < 11; ++k) w.g[k] = gf[k] / sf;
    return w;
}

inline long long align_up(long long v, long long a) { return (v + a - 1) / a * a; }

inline bool cam_ok(const v3d_gs_camera* c) {
    return c && c->width > 0 && c->height > 0 && c->tanfovx > 0.f && c->tanfovy > 0.f;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int v3d_gs_knn3(const float* xyz, int64_t n, float* out, v3d_stream_t stream) {
    V3D_REQUIRE(xyz && out && n >= 4, "v3d_gs_knn3: bad args (n >= 4 points)");
    hipLaunchKernelGGL(knn3_kernel, dim3(nblk(n)), dim3(NT), 0, ST, xyz, (long long)n, out);
    return v3d_check_launch("v3d_gs_knn3");
}

extern "C" int v3d_gs_preprocess_fwd(const float* xyz, const float* scale_raw, const float* rot_raw, const float* opacity_raw, const float* f_dc,
                                     int64_t P, const v3d_gs_camera* cam, float* means2d, float* conic_opacity, float* rgb, float* depth,
                                     int32_t* radii, int32_t* tiles_touched, int32_t* clamped, v3d_stream_t stream) {
    V3D_REQUIRE(xyz && scale_raw && rot_raw && opacity_raw && f_dc && means2d && conic_opacity && rgb && depth && radii && tiles_touched && clamped &&
                P > 0, "v3d_gs_preprocess_fwd: bad args");
    V3D_REQUIRE(cam_ok(cam), "v3d_gs_preprocess_fwd: bad camera (positive width, height, tan(fov/2))");
    const int gx = (cam->width + TILE - 1) / TILE, gy = (cam->height + TILE - 1) / TILE;
    hipLaunchKernelGGL(preprocess_fwd_kernel, dim3(nblk(P)), dim3(NT), 0, ST, (long long)P, xyz, scale_raw, rot_raw, opacity_raw, f_dc, *cam, gx, gy,
                       means2d, conic_opacity, rgb, depth, radii, tiles_touched, clamped);
    return v3d_check_launch("v3d_gs_preprocess_fwd");
}

extern "C" int64_t v3d_gs_scan_work_bytes(int64_t n) { return n < 0 ? -1 : 4 * ((n + SCAN_CHUNK - 1) / SCAN_CHUNK + 1); }

extern "C" int v3d_gs_scan(const int32_t* in, int64_t n, int32_t* out, void* work, int64_t work_bytes, v3d_stream_t stream) {
    V3D_REQUIRE(in && out && work && n > 0, "v3d_gs_scan: bad args");
    V3D_REQUIRE(work_bytes >= v3d_gs_scan_work_bytes(n), "v3d_gs_scan: work buffer too small (v3d_gs_scan_work_bytes)");
    const long long nb = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
    int32_t* bsum = (int32_t*)work;
    hipLaunchKernelGGL(scan_sums_kernel, dim3(nb), dim3(NT), 0, ST, in, (long long)n, bsum);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(NT), 0, ST, bsum, nb, out + n);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(NT), 0, ST, in, (long long)n, bsum, out);
    return v3d_check_launch("v3d_gs_scan");
}

extern "C" int v3d_gs_duplicate_keys(const float* means2d, const int32_t* radii, const float* depth, const int32_t* offsets, int64_t P,
                                     int32_t width, int32_t height, uint64_t* keys, uint32_t* vals, v3d_stream_t stream) {
    V3D_REQUIRE(means2d && radii && depth && offsets && keys && vals && P > 0 && width > 0 && height > 0, "v3d_gs_duplicate_keys: bad args");
    const int gx = (width + TILE - 1) / TILE, gy = (height + TILE - 1) / TILE;
    hipLaunchKernelGGL(duplicate_keys_kernel, dim3(nblk(P)), dim3(NT), 0, ST, (long long)P, means2d, radii, depth, offsets, gx, gy, keys, vals);
    return v3d_check_launch("v3d_gs_duplicate_keys");
}

static long long rs_blocks(long long n) { return (n + RS_CHUNK - 1) / RS_CHUNK; }

extern "C" int64_t v3d_gs_sort_work_bytes(int64_t n) {
    if (n <= 0) return n < 0 ? -1 : 0;
    const long long nc = (long long)RS_DIG * rs_blocks(n);
    return align_up(8 * n, 256) + align_up(4 * n, 256) + align_up(4 * (nc + 1), 256) + align_up(4 * (nc + 1), 256) +
           align_up(v3d_gs_scan_work_bytes(nc), 256);
}

extern "C" int v3d_gs_radix_sort_pairs(const uint64_t* keys_in, const uint32_t* vals_in, uint64_t* keys_out, uint32_t* vals_out, int64_t n,
                                       int32_t nbits, void* work, int64_t work_bytes, v3d_stream_t stream) {
    V3D_REQUIRE(keys_in && vals_in && keys_out && vals_out && work && n > 0, "v3d_gs_radix_sort_pairs: bad args");
    V3D_REQUIRE(nbits >= 1 && nbits <= 64, "v3d_gs_radix_sort_pairs: 1 <= nbits <= 64");
    V3D_REQUIRE(work_bytes >= v3d_gs_sort_work_bytes(n), "v3d_gs_radix_sort_pairs: work buffer too small (v3d_gs_sort_work_bytes)");
    V3D_REQUIRE((const void*)keys_in != (void*)keys_out && (const void*)vals_in != (void*)vals_out, "v3d_gs_radix_sort_pairs: not in place");
    const long long nb = rs_blocks(n), nc = (long long)RS_DIG * nb;
    char* p = (char*)work;
    uint64_t* ktmp = (uint64_t*)p; p += align_up(8 * n, 256);
    uint32_t* vtmp = (uint32_t*)p; p += align_up(4 * n, 256);
    int32_t* counts = (int32_t*)p; p += align_up(4 * (nc + 1), 256);
    int32_t* offs = (int32_t*)p; p += align_up(4 * (nc + 1), 256);
    void* swork = p;
    const int passes = (nbits + RS_BITS - 1) / RS_BITS;
    const uint64_t* ks = keys_in;
    const uint32_t* vs = vals_in;
    for (int pass = 0; pass < passes; ++pass) {
        const bool to_out = ((passes - 1 - pass) % 2) == 0;
        uint64_t* kd = to_out ? keys_out : ktmp;
        uint32_t* vd = to_out ? vals_out : vtmp;
        const int shift = pass * RS_BITS;
        // the last digit ends at bit nbits: key bits above it take no part, so keys that differ only there keep their input order
        const unsigned dmask = (1u << (nbits - shift < RS_BITS ? nbits - shift : RS_BITS)) - 1u;
        hipLaunchKernelGGL(radix_count_kernel, dim3(nb), dim3(NT), 0, ST, ks, (long long)n, shift, dmask, nb, counts);
        int rc = v3d_gs_scan(counts, nc, offs, swork, v3d_gs_scan_work_bytes(nc), stream);
        if (rc) return rc;
        hipLaunchKernelGGL(radix_scatter_kernel, dim3(nb), dim3(NT), 0, ST, ks, vs, (long long)n, shift, dmask, nb, offs, kd, vd);
        ks = kd;
        vs = vd;
    }
    return v3d_check_launch("v3d_gs_radix_sort_pairs");
}

extern "C" int v3d_gs_tile_ranges(const uint64_t* keys_sorted, const uint32_t* vals_sorted, int64_t n_inst, const float* means2d, const int32_t* radii,
                                  const int32_t* offsets, int32_t width, int32_t height, int32_t* ranges, int32_t* inst_pos, v3d_stream_t stream) {
    V3D_REQUIRE(means2d && radii && offsets && ranges && width > 0 && height > 0 && n_inst >= 0, "v3d_gs_tile_ranges: bad args");
    V3D_REQUIRE(n_inst == 0 || (keys_sorted && vals_sorted && inst_pos), "v3d_gs_tile_ranges: null instance arrays");
    const int gx = (width + TILE - 1) / TILE, gy = (height + TILE - 1) / TILE;
    hipError_t e = hipMemsetAsync(ranges, 0, sizeof(int32_t) * 2 * (size_t)gx * gy, ST);
    if (e != hipSuccess) {
        v3d_set_error("v3d_gs_tile_ranges: hipMemsetAsync: %s", hipGetErrorString(e));
        return V3D_ERR_LAUNCH;
    }
    if (n_inst > 0)
        hipLaunchKernelGGL(tile_ranges_kernel, dim3(nblk(n_inst)), dim3(NT), 0, ST, keys_sorted, vals_sorted, (long long)n_inst, means2d, radii, offsets,
                           gx, gy, ranges, inst_pos);
    return v3d_check_launch("v3d_gs_tile_ranges");
}

extern "C" int v3d_gs_render_fwd(const int32_t* ranges, const uint32_t* vals_sorted, const float* means2d, const float* conic_opacity, const float* rgb,
                                 const v3d_gs_camera* cam, float* out_img, float* final_T, int32_t* n_contrib, v3d_stream_t stream) {
    V3D_REQUIRE(ranges && means2d && conic_opacity && rgb && out_img && final_T && n_contrib, "v3d_gs_render_fwd: bad args");
    V3D_REQUIRE(cam_ok(cam), "v3d_gs_render_fwd: bad camera");
    const int gx = (cam->width + TILE - 1) / TILE, gy = (cam->height + TILE - 1) / TILE;
    hipLaunchKernelGGL(render_fwd_kernel, dim3(gx * gy), dim3(NT), 0, ST, ranges, vals_sorted, means2d, conic_opacity, rgb, *cam, gx, out_img, final_T,
                       n_contrib);
    return v3d_check_launch("v3d_gs_render_fwd");
}

extern "C" int v3d_gs_render_bwd(const int32_t* ranges, const uint32_t* vals_sorted, const float* means2d, const float* conic_opacity, const float* rgb,
                                 const v3d_gs_camera* cam, const float* final_T, const int32_t* n_contrib, const float* dL_dimg, float* inst_grads,
                                 v3d_stream_t stream) {
    V3D_REQUIRE(ranges && means2d && conic_opacity && rgb && final_T && n_contrib && dL_dimg, "v3d_gs_render_bwd: bad args");
    V3D_REQUIRE(cam_ok(cam), "v3d_gs_render_bwd: bad camera");
    const int gx = (cam->width + TILE - 1) / TILE, gy = (cam->height + TILE - 1) / TILE;
    hipLaunchKernelGGL(render_bwd_kernel, dim3(gx * gy), dim3(NT), 0, ST, ranges, vals_sorted, means2d, conic_opacity, rgb, *cam, gx, final_T, n_contrib,
                       dL_dimg, inst_grads);
    return v3d_check_launch("v3d_gs_render_bwd");
}

extern "C" int v3d_gs_reduce_instance_grads(const float* inst_grads, const int32_t* offsets, const int32_t* inst_pos, int64_t P, float* grads9,
                                            v3d_stream_t stream) {
    V3D_REQUIRE(offsets && grads9 && P > 0, "v3d_gs_reduce_instance_grads: bad args");
    hipLaunchKernelGGL(reduce_grads_kernel, dim3(nblk(P)), dim3(NT), 0, ST, inst_grads, offsets, inst_pos, (long long)P, grads9);
    return v3d_check_launch("v3d_gs_reduce_instance_grads");
}

extern "C" int v3d_gs_preprocess_bwd(const float* xyz, const float* scale_raw, const float* rot_raw, const float* opacity_raw, int64_t P,
                                     const v3d_gs_camera* cam, const int32_t* radii, const int32_t* clamped, const float* grads9, float* d_xyz,
                                     float* d_scale_raw, float* d_rot_raw, float* d_opacity_raw, float* d_f_dc, float* d_means2d, v3d_stream_t stream) {
    V3D_REQUIRE(xyz && scale_raw && rot_raw && opacity_raw && radii && clamped && grads9 && d_xyz && d_scale_raw && d_rot_raw && d_opacity_raw &&
                d_f_dc && d_means2d && P > 0, "v3d_gs_preprocess_bwd: bad args");
    V3D_REQUIRE(cam_ok(cam), "v3d_gs_preprocess_bwd: bad camera");
    hipLaunchKernelGGL(preprocess_bwd_kernel, dim3(nblk(P)), dim3(NT), 0, ST, (long long)P, xyz, scale_raw, rot_raw, opacity_raw, *cam, radii, clamped,
                       grads9, d_xyz, d_scale_raw, d_rot_raw, d_opacity_raw, d_f_dc, d_means2d);
    return v3d_check_launch("v3d_gs_preprocess_bwd");
}

extern "C" int64_t v3d_gs_ssim_work_floats(int32_t C, int32_t H, int32_t W) {
    if (C <= 0 || H <= 0 || W <= 0) return -1;
    const long long chw = (long long)C * H * W;
    return 13 * chw + 2 * (long long)nblk(chw);        // 5 fp64 moment maps, 3 gradient maps, per-block partial sums
}

extern "C" int v3d_gs_ssim_l1_fwd(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, float lambda_dssim, float* work,
                                  int64_t work_floats, float* out3, v3d_stream_t stream) {
    V3D_REQUIRE(img && gt && work && out3 && C > 0 && H > 0 && W > 0, "v3d_gs_ssim_l1_fwd: bad args");
    V3D_REQUIRE(work_floats >= v3d_gs_ssim_work_floats(C, H, W), "v3d_gs_ssim_l1_fwd: work buffer too small (v3d_gs_ssim_work_floats)");
    const long long chw = (long long)C * H * W, nb = nblk(chw);
    const Win win = ssim_window();
    V3D_REQUIRE(((uintptr_t)work & 7) == 0, "v3d_gs_ssim_l1_fwd: work must be 8-byte aligned");
    double* h5 = (double*)work;
    float* gm = work + 10 * chw;
    float* part = work + 13 * chw;
    hipLaunchKernelGGL((ssim_hblur_kernel<0, double>), dim3(nb), dim3(NT), 0, ST, img, gt, (long long)C, (int)H, (int)W, win, h5);
    hipLaunchKernelGGL(ssim_vfwd_kernel, dim3(nb), dim3(NT), 0, ST, img, gt, h5, (long long)C, (int)H, (int)W, win, gm, part);
    hipLaunchKernelGGL(ssim_final_kernel, dim3(1), dim3(NT), 0, ST, part, nb, chw, lambda_dssim, out3);
    return v3d_check_launch("v3d_gs_ssim_l1_fwd");
}

extern "C" int v3d_gs_ssim_l1_bwd(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, float lambda_dssim, float* work,
                                  int64_t work_floats, const float* dloss, float* grad, v3d_stream_t stream) {
    V3D_REQUIRE(img && gt && work && dloss && grad && C > 0 && H > 0 && W > 0, "v3d_gs_ssim_l1_bwd: bad args");
    V3D_REQUIRE(work_floats >= v3d_gs_ssim_work_floats(C, H, W), "v3d_gs_ssim_l1_bwd: work buffer too small (v3d_gs_ssim_work_floats)");
    const long long chw = (long long)C * H * W, nb = nblk(chw);
    const Win win = ssim_window();
    float* h3 = work;               // (the forward's five blurred maps are no longer needed)
    const float* gm = work + 10 * chw;
    hipLaunchKernelGGL((ssim_hblur_kernel<1, float>), dim3(nb), dim3(NT), 0, ST, gm, (const float*)nullptr, (long long)C, (int)H, (int)W, win, h3);
    hipLaunchKernelGGL(ssim_vbwd_kernel, dim3(nb), dim3(NT), 0, ST, img, gt, h3, (long long)C, (int)H, (int)W, win, lambda_dssim, dloss, grad);
    return v3d_check_launch("v3d_gs_ssim_l1_bwd");
}
