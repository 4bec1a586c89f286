// Sampler-loop kernels of the ancestral / DPM++ / linear-multistep samplers (gfx950): counter-based Gaussian noise fused into an add, and a
// small fp32 linear combination.  Built WITHOUT -ffast-math (v3d_amd/build.py FILE_FLAGS): logf / sincospif must be the precise library
// functions, not the approximate forms fast-math lets the compiler substitute.
//
// Noise spec (v3d_randn_add; tests/philox_ref.py restates it in numpy and pins it to the Random123 known-answer vectors):
//   g      = flat index of the element in the UNSHARDED [(b T_global), C, H, W] tensor; local row r = b T_local + t is global row
//            b T_global + t0 + t, so every frame shard draws exactly the numbers of its rows of the unsharded tensor
//   q = g >> 2, lane = g & 3
//   (r0, r1, r2, r3) = Philox4x32_10(counter = (q & 0xffffffff, q >> 32, call, 0), key = (seed & 0xffffffff, seed >> 32))
//                      M0 = 0xD2511F53, M1 = 0xCD9E8D57, W0 = 0x9E3779B9, W1 = 0xBB67AE85 (Salmon et al., SC'11)
//   u(r)   = ((r >> 8) + 0.5) * 2^-24, evaluated in fp32 (round to nearest even: the +0.5 survives below 2^23, above it the sum rounds;
//            u is never 0, and u = 1 only for r >> 8 = 2^24 - 1, which gives rho = 0)
//   rho(a) = sqrt(-2 ln u(a))
//   lanes 0, 1: rho(r0) cos(2 pi u(r1)), rho(r0) sin(2 pi u(r1)); lanes 2, 3: the same with r2, r3   (Box-Muller)
// One thread makes one group of 4 lanes = 4 consecutive elements (row_elems % 4 == 0 keeps a group inside one row) with one 16-byte load
// and one 16-byte store.
#include "common.h"

namespace {

inline unsigned nblocks(long long n, int per_block = 256, long long cap = 1 << 20) {
    long long b = (n + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (unsigned)b;
}

__device__ __forceinline__ u32x4 philox4x32_10(u32x4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = u32x4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    }
    return c;
}

__device__ __forceinline__ float unit_open(uint32_t r) { return ((float)(r >> 8) + 0.5f) * 5.9604644775390625e-08f; }   // 2^-24

__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
    const float rho = sqrtf(-2.0f * logf(unit_open(a)));
    float s, c;
    sincospif(2.0f * unit_open(b), &s, &c);
    z0 = rho * c;
    z1 = rho * s;
}

__global__ void randn_add_kernel(const float* x, float scale, uint32_t k0, uint32_t k1, uint32_t call, float* out,
                                 long long rows, long long T_local, long long T_global, long long t0, long long row_groups) {
    const long long total = rows * row_groups;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / row_groups, e4 = i - r * row_groups;
        const long long b = r / T_local, t = r - b * T_local;
        const unsigned long long q = (unsigned long long)((b * T_global + t0 + t) * row_groups + e4);     // = g >> 2
        const u32x4 ph = philox4x32_10(u32x4{(uint32_t)q, (uint32_t)(q >> 32), call, 0u}, k0, k1);
        float z0, z1, z2, z3;
        box_muller(ph.x, ph.y, z0, z1);
        box_muller(ph.z, ph.w, z2, z3);
        const f32x4 z = {z0, z1, z2, z3};
        f32x4 v = x ? *reinterpret_cast<const f32x4*>(x + 4 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
        v += scale * z;
        *reinterpret_cast<f32x4*>(out + 4 * i) = v;
    }
}

struct LinComb {
    const float* src[6];
    float coef[6];
    int nterms;
};

// out[i] = sum_k coef[k] src[k][i], terms added in order k = 0, 1, ...  No __restrict__: out may be one of the sources (every element is
// read and then written by the same thread).  VEC: 16-byte accesses (n % 4 == 0, all pointers 16-byte aligned).
template <bool VEC>
__global__ void lincomb_kernel(LinComb p, float* out, long long n) {
    const long long m = VEC ? n / 4 : n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long long)gridDim.x * blockDim.x) {
        if constexpr (VEC) {
            f32x4 acc = p.coef[0] * *reinterpret_cast<const f32x4*>(p.src[0] + 4 * i);
            for (int k = 1; k < p.nterms; ++k) acc += p.coef[k] * *reinterpret_cast<const f32x4*>(p.src[k] + 4 * i);
            *reinterpret_cast<f32x4*>(out + 4 * i) = acc;
        } else {
            float acc = p.coef[0] * p.src[0][i];
            for (int k = 1; k < p.nterms; ++k) acc += p.coef[k] * p.src[k][i];
            out[i] = acc;
        }
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int v3d_randn_add(const float* x, float scale, uint64_t seed, uint32_t call, float* out, int64_t B, int64_t T_local,
                             int64_t T_global, int64_t t0, int64_t row_elems, v3d_stream_t stream) {
    V3D_REQUIRE(out && B > 0 && T_local > 0 && row_elems > 0 && t0 >= 0 && t0 + T_local <= T_global, "v3d_randn_add: bad args");
    V3D_REQUIRE(row_elems % 4 == 0, "v3d_randn_add: row_elems must be a multiple of 4");
    V3D_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "v3d_randn_add: pointers must be 16-byte aligned");
    const long long rows = B * T_local, row_groups = row_elems / 4;
    hipLaunchKernelGGL(randn_add_kernel, dim3(nblocks(rows * row_groups)), dim3(256), 0, ST, x, scale, (uint32_t)seed, (uint32_t)(seed >> 32),
                       call, out, rows, (long long)T_local, (long long)T_global, (long long)t0, row_groups);
    return v3d_check_launch("v3d_randn_add");
}

extern "C" int v3d_lincomb_f32(const float* const* src, const float* coef, int32_t nterms, float* out, int64_t n, v3d_stream_t stream) {
    V3D_REQUIRE(src && coef && out && n > 0 && nterms >= 1 && nterms <= 6, "v3d_lincomb_f32: bad args (1 <= nterms <= 6)");
    LinComb p = {};
    uintptr_t align = (uintptr_t)out;
    for (int k = 0; k < nterms; ++k) {
        V3D_REQUIRE(src[k], "v3d_lincomb_f32: null source");
        p.src[k] = src[k];
        p.coef[k] = coef[k];
        align |= (uintptr_t)src[k];
    }
    p.nterms = nterms;
    if (n % 4 == 0 && (align & 15) == 0)
        hipLaunchKernelGGL(lincomb_kernel<true>, dim3(nblocks(n / 4)), dim3(256), 0, ST, p, out, (long long)n);
    else
        hipLaunchKernelGGL(lincomb_kernel<false>, dim3(nblocks(n)), dim3(256), 0, ST, p, out, (long long)n);
    return v3d_check_launch("v3d_lincomb_f32");
}
