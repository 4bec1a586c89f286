// v3d_ff_fused: FeedForward(GEGLU) of the transformer blocks with the 4x-wide hidden tensor kept on the CU (gfx950).
//
// Reference: sgm/modules/attention.py:82-113 (GEGLU: Linear(C, 2*4C) -> value * gelu(gate); FeedForward: GEGLU, Dropout, Linear(4C, C)).
// The unfused pair (v3d_gemm with the GEGLU epilogue, then v3d_gemm) writes and re-reads a 377 MB hidden tensor per block at the
// 64x64 level; the second GEMM streams it at ~2.9 TB/s and the first one's epilogue (one GELU per output + the stores) costs as much
// as its main loop.  Here a block of 128 pixel rows walks the hidden dimension in slabs of 32 channels:
//   stage A   S[64 x 32px] = W1 slab (64 packed rows: 2 fragments of 16 value + 16 gate rows) . x^T   (x fragments stay in registers)
//   stage G   h[32 ch] = (S_value + b) * gelu(S_gate + b)  - the lane now holds 8 hidden values of its pixel per fragment
//   stage B   out[C x 32px] += W2[:, slab] . h               (h is the MFMA operand straight from those registers: the K order of
//                                                             W2 inside a slab is permuted at pack time to the order the lanes hold)
// All MFMAs are v_mfma_f32_32x32x16_bf16: with a 32-pixel wave tile every LDS fragment read (1 KiB) feeds 32 cycles of matrix work,
// twice what 16x16x32 fragments give - the first version of this kernel was LDS-read bound in stage A.
// 4 waves, ONE per SIMD (512-VGPR budget: 160 output accumulators + 80 resident x fragments + 2 x 32 slab accumulators).  The three
// stages are software-pipelined across slabs: tick j runs A(j+1), G(j) and B(j-1), which are mutually independent, so the GELU VALU
// work and the LDS-DMA issue of the next weights sit in the shadow of the MFMAs of the other two stages.  Both weight streams go
// through double-buffered LDS slabs (buffer-load LDS-DMA, one barrier per tick); the weight stream is block-independent, so it
// runs across row-block boundaries, where the last B of a block shares a tick with the first A of the next.
#include "common.h"

namespace {

struct FFP {
    const bf16_t* x;
    const bf16_t* W1;
    const bf16_t* W2;
    const float* b1;
    const float* b2;
    const bf16_t* res1;
    const bf16_t* res2;
    const float* coef;
    bf16_t* out;
    long long M, ldx, ldr1, ldr2, ldo, coef_rpg;
    float c_acc, c_res1, c_res2;
    int hidden;
    float ln_eps;        // <LN> kernels: LayerNorm (no affine) of the input rows in registers before the first GEMM
    unsigned w1_bytes, w2_bytes;
};

template <int I, int N, typename F>
__device__ __forceinline__ void ff_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        ff_static_for<I + 1, N>(f);
    }
}

// Issue order of one tick (a single scheduling region): every MFMA is followed by one LDS fragment read, its share of the GELU
// VALU work and - every 4th - one LDS-DMA piece with its scalar address, so that a wave that is alone on its SIMD keeps the
// matrix pipe fed while it issues everything else in the MFMA shadows (left alone the scheduler emits DMAs, MFMAs, VALU en bloc).
template <int NMFMA, int NVALU>
__device__ __forceinline__ void ff_tick_pipeline() {
    __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
    ff_static_for<0, NMFMA>([&](auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        if constexpr (i % 4 == 1) {
            __builtin_amdgcn_sched_group_barrier(0x004, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x402, NVALU, 0);
    });
}

__device__ __forceinline__ int ff_swz(int row) { return (0x78 >> (((row >> 2) & 3) * 2)) & 3; }   // 64-byte LDS rows, see gemm.hip

template <int C, bool LN>
__global__ __launch_bounds__(256, 1) void ff_fused_kernel(FFP p) {
    constexpr int NT = C / 32;                 // 32-k LDS stages of a W1 slab
    constexpr int NK = C / 16;                 // k16 steps of stage A = resident x fragments
    constexpr int NO = C / 32;                 // 32-channel output fragments
    constexpr int W1_STAGE = 64 * 64;          // 64 packed rows x 64 B (32 k)
    constexpr int W1_BYTES = NT * W1_STAGE;
    constexpr int W2_BYTES = C * 64;           // C output rows x 64 B (the slab's 32 hidden channels)
    constexpr int NP1 = NT * 4, NP2 = C / 16;  // 1-KiB DMA pieces per slab
    static_assert(NP1 % 4 == 0 && NP2 % 4 == 0, "pieces per wave");
    constexpr int PPW1 = NP1 / 4, PPW2 = NP2 / 4;
    constexpr int SROW = 128 + 16;             // staged row: 64 channels + pad
    constexpr int STAGE_REGION = 32 * SROW;
    static_assert(NO % 2 == 0, "staging geometry");
    constexpr int RING = 2 * W1_BYTES + 3 * W2_BYTES;   // W1 double-buffered, W2 three deep (see the tick description)
    constexpr int B2_OFF = RING + 4 * STAGE_REGION;   // b2 lives in LDS: the epilogue's only global loads are then its prefetches
    constexpr int LDS_BYTES = B2_OFF + C * 4;
    static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
    __shared__ __attribute__((aligned(1024))) unsigned char lds[LDS_BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    unsigned char* const w1ring = lds;
    unsigned char* const w2ring = lds + 2 * W1_BYTES;
    unsigned char* stage = lds + RING + wave * STAGE_REGION;

    // ---- weight-slab loader: 1-KiB pieces (16 rows x 64 B) whose LDS image is: lane l -> row l >> 2, 16-byte chunk (l & 3) ^ swz(row)
    const bufrsrc_t rsW1 = make_rsrc(p.W1, p.w1_bytes);
    const bufrsrc_t rsW2 = make_rsrc(p.W2, p.w2_bytes);
    // piece q = wave + 4 i of W1 is LDS stage i, rows 16 wave ..; of W2 rows 16 (wave + 4 i) ..: one base VGPR per stream, the rest is
    // a scalar offset (NOT the instruction's immediate: that one is added to the LDS address as well)
    // the packed weights are stored in DMA-piece order (packing.py ff_dma_tile_index: 16 rows x 64 B, LDS swizzle pre-applied), so a
    // piece is one contiguous KiB: lane l reads bytes 16 l .. 16 l + 15 of it (row-strided 64-byte segments DMA'd 24 % slower)
    const unsigned voff1 = (unsigned)(wave * 1024 + lane * 16);
    const unsigned voff2 = (unsigned)(wave * 1024 + lane * 16);
    const int w2_step = 4096;
    const int nslab = p.hidden / 32;
    int ld1 = 0, ld2 = 0;   // next slab of each weight stream (both wrap: the stream does not depend on the row block)
    // LDS fragment of 32 rows x 16 k out of 64-byte rows: row l31, logical 16-byte chunk 2 kk + hi
    const int foff0 = l31 * 64 + (((0 + hi) ^ ff_swz(l31)) * 16);
    const int foff1 = l31 * 64 + (((2 + hi) ^ ff_swz(l31)) * 16);
    const long long nblocks = p.M / 128;

    f32x16 acc2[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[o][r] = 0.f;
    f32x16 sA[2][2];                   // slab accumulators [slab parity][row fragment]
    bf16x8 hh[2][2];                   // GEGLU outputs      [slab parity][row fragment = k16 step of stage B]
    bf16x8 xr[NK];                     // the wave's 32 input rows as MFMA operand fragments, resident for the whole block

    auto load_x = [&](long long blk) __attribute__((always_inline)) {
        const bf16_t* xz = p.x + (blk * 128 + wave * 32 + l31) * p.ldx + hi * 8;
#pragma unroll
        for (int k = 0; k < NK; ++k) xr[k] = *reinterpret_cast<const bf16x8*>(xz + k * 16);
    };

    // ---- one tick = NS issue slots, each closed by a scheduling fence: [MFMA] [LDS fragment read NPD slots ahead] [every 4th: one
    //      LDS-DMA piece] [one third of a GELU evaluation].  A wave alone on its SIMD has nobody to cover its issue gaps, so the order
    //      is fixed here instead of left to the scheduler (which emits the DMAs, the MFMAs and the VALU work en bloc).
    //   stage B (parity PB): out += W2[:, slab] . h, fragment q = a NO + o                       slots 0 .. 2 NO - 1
    //   stage A (parity PA): S = W1 slab . x^T, fragment q = 4 t + 2 kk + a                        the next 4 NT slots
    //   stage G (parity PG): the MFMA rows of a fragment are 8 g + 4 hi + c (g = reg >> 2, c = reg & 3): g even = value, g odd =
    //                        gate of hidden channel 8 (g >> 1) + 4 hi + c -> the lane's 8 values are one k16 operand of stage B
    //   DMA:                 W1 slab ld1 -> w1ring[PD] (read next tick), W2 slab ld2 -> the W2 slot two ticks ahead of its use (D2)
    // A parity of -1 switches the stage off.  W2 is three slots deep: the slab DMA'd in tick j is first read in tick j + 2, so its
    // pieces (the last five a wave issues in a tick) may still be in flight at the tick's barrier - the wait there is vmcnt(5), and the
    // LDS-DMA stream, which is what a tick ends up waiting for, never drains (the alternative use of the third slot, prefetching the
    // next tick's first fragments ahead of the barrier, needs vmcnt(0) and measured 6 % slower).
    constexpr int NPD = 4;             // LDS fragment reads run this many slots ahead of their MFMAs
    bf16x8 wf[NPD];                    // (carried across ticks: a tick prefetches the next one's first fragments)
    int w2_wr_slot = 0, w2_rd_slot = 0;
    auto tick = [&](auto pa_c, auto pg_c, auto pb_c, auto pd_c, auto d2_c, int j) __attribute__((always_inline)) {
        constexpr int PA = decltype(pa_c)::value, PG = decltype(pg_c)::value, PB = decltype(pb_c)::value, PDM = decltype(pd_c)::value;
        constexpr bool D2 = decltype(d2_c)::value != 0;
        constexpr int NB = PB >= 0 ? 2 * NO : 0, NA = PA >= 0 ? 4 * NT : 0, NS = 2 * NO + 4 * NT;
        // the slab accumulators start from b1 (row 8 g + 4 hi + c of fragment a <-> register 4 g + c): eight global loads at the tick
        // top (issued inside the tick they queue behind ~1500 cycles of LDS-DMA traffic), moved into the accumulators in the four
        // slots before stage A's first MFMA.  (b1 riding its W1 slab as an exec-masked
        // LDS-DMA piece, read from LDS in slots 8..15, measured 500 against 468 us: it lengthens stage B's slots by more than it saves.)
        float4 bu[4], bv[4];
        const unsigned char* bz = reinterpret_cast<const unsigned char*>(p.b1 + (j == nslab ? 0 : j + 1) * 64 + hi * 4);
        if constexpr (PA >= 0) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                bu[g] = *reinterpret_cast<const float4*>(bz + g * 32);
                bv[g] = *reinterpret_cast<const float4*>(bz + 128 + g * 32);
            }
        }
        int so1 = 0, so2 = 0, w2wr = 0;
        if constexpr (PDM >= 0) {
            so1 = ld1 * 64 * C * 2;
            if (++ld1 == nslab) ld1 = 0;
        }
        if constexpr (D2) {
            so2 = ld2 * W2_BYTES;
            if (++ld2 == nslab) ld2 = 0;
            w2wr = w2_wr_slot * W2_BYTES;
            if (++w2_wr_slot == 3) w2_wr_slot = 0;
        }
        // stage B reads the W2 slot w2_rd_slot (runtime: 3 does not divide the 2-tick unroll)
        const int fb0 = foff0 + w2_rd_slot * W2_BYTES, fb1 = foff1 + w2_rd_slot * W2_BYTES;
        if constexpr (PB >= 0) {
            if (++w2_rd_slot == 3) w2_rd_slot = 0;
        }
        auto rd = [&](auto fc) __attribute__((always_inline)) -> bf16x8 {
            constexpr int f = decltype(fc)::value;
            if constexpr (f < NB)
                return *reinterpret_cast<const bf16x8*>(w2ring + (f % NO) * 2048 + ((f / NO) ? fb1 : fb0));
            else {
                constexpr int q = f - NB;
                return *reinterpret_cast<const bf16x8*>(w1ring + (PA < 0 ? 0 : PA) * W1_BYTES + (q >> 2) * W1_STAGE + (q & 1) * 2048 +
                                                        (((q >> 1) & 1) ? foff1 : foff0));
            }
        };
        // the tick's first fragments, visible only after the barrier that just passed
        ff_static_for<0, NPD>([&](auto fc) __attribute__((always_inline)) {
            if constexpr (decltype(fc)::value < NB + NA) wf[decltype(fc)::value] = rd(fc);
        });
        if constexpr (PA >= 0 && NB < 16) {   // no stage B to wait behind (first tick of a block): once per block, stall accepted
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                sA[PA][0][4 * g] = bu[g].x; sA[PA][0][4 * g + 1] = bu[g].y; sA[PA][0][4 * g + 2] = bu[g].z; sA[PA][0][4 * g + 3] = bu[g].w;
                sA[PA][1][4 * g] = bv[g].x; sA[PA][1][4 * g + 1] = bv[g].y; sA[PA][1][4 * g + 2] = bv[g].z; sA[PA][1][4 * g + 3] = bv[g].w;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        float gx = 0.f, gz = 0.f, gq = 0.f, hprev = 0.f;
        u32x4 hw0 = {0, 0, 0, 0}, hw1 = {0, 0, 0, 0};
        auto gstep = [&](auto ms_c) __attribute__((always_inline)) {
            {
                constexpr int ms = decltype(ms_c)::value, e = ms / 3, st = ms % 3;
                if constexpr (e < 16) {
                    constexpr int a = e / 8, idx = e % 8, vreg = idx < 4 ? idx : idx + 4, greg = vreg + 4;
                    if constexpr (st == 0) {
                        gx = sA[PG][a][greg];
                        gz = fminf(fabsf(gx) * 0.70710678118654752440f, 4.0f);
                        gq = __builtin_fmaf(-1.664338751e-02f, gz, 1.293501013e-01f);
                        gq = __builtin_fmaf(gq, gz, 9.298687989e-01f);
                    } else if constexpr (st == 1) {
                        gq = __builtin_fmaf(gq, gz, 1.625731271e+00f);
                        gq = __builtin_fmaf(gq, gz, 1.0f);
                        gq = __builtin_amdgcn_exp2f(-gq);
                    } else {
                        const float hv = sA[PG][a][vreg] * (fmaxf(gx, 0.0f) - fabsf(gx) * gq);
                        if constexpr (idx & 1) {
                            if constexpr (a == 0) hw0[idx >> 1] = pack2bf(hprev, hv);
                            else hw1[idx >> 1] = pack2bf(hprev, hv);
                        } else
                            hprev = hv;
                    }
                }
            }
        };
        constexpr int G_FRONT = 6;     // GELU pieces executed at the tick top, beside the bias loads
        if constexpr (PG >= 0) {
            ff_static_for<0, G_FRONT>([&](auto mc) __attribute__((always_inline)) { gstep(mc); });
            __builtin_amdgcn_sched_barrier(0);
        }
        ff_static_for<0, NS>([&](auto ic) __attribute__((always_inline)) {
            constexpr int i = decltype(ic)::value;
            if constexpr (PA >= 0 && NB >= 16 && i + 4 >= NB && i < NB) {
                constexpr int g = i + 4 - NB;
                sA[PA][0][4 * g] = bu[g].x; sA[PA][0][4 * g + 1] = bu[g].y; sA[PA][0][4 * g + 2] = bu[g].z; sA[PA][0][4 * g + 3] = bu[g].w;
                sA[PA][1][4 * g] = bv[g].x; sA[PA][1][4 * g + 1] = bv[g].y; sA[PA][1][4 * g + 2] = bv[g].z; sA[PA][1][4 * g + 3] = bv[g].w;
            }
            if constexpr (i < NB + NA) {
                const bf16x8 w = wf[i % NPD];
                if constexpr (i < NB) {
                    constexpr int bo = i % NO, ba = i / NO;
                    acc2[bo] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w, hh[PB < 0 ? 0 : PB][ba], acc2[bo], 0, 0, 0);
                }
                else {
                    constexpr int q = i - NB;
                    sA[PA < 0 ? 0 : PA][q & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w, xr[q >> 1], sA[PA < 0 ? 0 : PA][q & 1], 0, 0, 0);
                }
                if constexpr (i + NPD < NB + NA) wf[i % NPD] = rd(std::integral_constant<int, i + NPD>{});
            }
            if constexpr ((PDM >= 0 || D2) && i % 4 == 1) {
                constexpr int k = i / 4;
                if constexpr (k < PPW1 && PDM >= 0)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW1, (__attribute__((address_space(3))) void*)(w1ring + PDM * W1_BYTES + k * W1_STAGE + wave * 1024),
                                                             16, (int)voff1, so1 + k * 4096, 0, 0);
                else if constexpr (k >= PPW1 && k < PPW1 + PPW2 && D2)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW2, (__attribute__((address_space(3))) void*)(w2ring + w2wr + (wave + 4 * (k - PPW1)) * 1024),
                                                             16, (int)voff2, so2 + (k - PPW1) * w2_step, 0, 0);
            }
            // stage G: 16 GELUs x 3 pieces over the tick's slots, plain fp32 (packed fp32 beside MFMAs costs more than it saves) and as
            // few issue slots as the bf16 result allows - a wave alone on its SIMD hides ~5 instructions per 32x32x16 MFMA:
            //   gelu(x) = relu(x) - |x| 2^-(z Q(z) + 1),  z = min(|x| / sqrt2, 4),  0.5 erfc(z) = 2^-(z Q(z) + 1)
            // Q: degree-3 fit of -log2(erfc(z)) / z weighted for the GELU error (|error| <= 8.6e-6 in fp32 Horner; the value is rounded
            // to bf16, 4e-3 relative, right after).  11 VALU + 1 transcendental per value.
            // the 48 GELU pieces: G_FRONT of them at the tick top, the rest spread evenly over the slots
            if constexpr (PG >= 0) {
                constexpr int NSTEP = 48 - G_FRONT;
                if constexpr (i == 0 || (NSTEP * i) / NS != (NSTEP * (i - 1)) / NS) gstep(std::integral_constant<int, G_FRONT + (NSTEP * i) / NS>{});
            }
            __builtin_amdgcn_sched_barrier(0);
        });
        if constexpr (PG >= 0) {
            hh[PG][0] = __builtin_bit_cast(bf16x8, hw0);
            hh[PG][1] = __builtin_bit_cast(bf16x8, hw1);
        }
        // this wave's share of the next weights (and x / residual prefetches) has landed, but for this tick's five W2 pieces: they are
        // first read two ticks later, behind the next barrier
        if constexpr (D2) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                      // ... everyone's has, and every LDS read of this tick was consumed
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using IX = std::integral_constant<int, -1>;

    // ---- prologue: W1(0), W1(1), W2(0) in flight (as the ticks before a block would have left them), first x block, A(0) alone
    long long blk = blockIdx.x;
    if (tid < C / 4) reinterpret_cast<float4*>(lds + B2_OFF)[tid] = reinterpret_cast<const float4*>(p.b2)[tid];
    ff_static_for<0, 2 * PPW1>([&](auto ic) __attribute__((always_inline)) {
        constexpr int k = decltype(ic)::value % PPW1, par = decltype(ic)::value / PPW1;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW1, (__attribute__((address_space(3))) void*)(w1ring + par * W1_BYTES + k * W1_STAGE + wave * 1024), 16,
                                                 (int)voff1, par * 64 * C * 2 + k * 4096, 0, 0);
    });
    ld1 = 2;
    ff_static_for<0, PPW2>([&](auto ic) __attribute__((always_inline)) {
        constexpr int k = decltype(ic)::value;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW2, (__attribute__((address_space(3))) void*)(w2ring + (wave + 4 * k) * 1024), 16, (int)voff2,
                                                 k * w2_step, 0, 0);
    });
    ld2 = 1;
    w2_wr_slot = 1;
    load_x(blk);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (LN) ln_rows_inplace<NK>(xr, p.ln_eps);
    __builtin_amdgcn_s_barrier();
    tick(I0{}, IX{}, IX{}, IX{}, I0{}, -1);

    // residual rows of one epilogue pass (64 channels): res1 coalesced (row c >> 3, 16-byte chunk c & 7), res2 in the MFMA layout
    u32x4 r1[2][4];
    u32x2 r2[2][8];
    auto fetch_res = [&](long long mw0_, int ps, u32x4 (&q1)[4], u32x2 (&q2)[8]) __attribute__((always_inline)) {
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));   // keep the address arithmetic out of the block loop's live ranges (see the epilogue)
        if (p.res1) {
            const bf16_t* rz = p.res1 + mw0_ * p.ldr1 + ps * 64;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int c = it * 64 + lane_e;
                q1[it] = *reinterpret_cast<const u32x4*>(rz + (long long)(c >> 3) * p.ldr1 + (c & 7) * 8);
            }
        } else {
#pragma unroll
            for (int it = 0; it < 4; ++it) q1[it] = u32x4{0, 0, 0, 0};
        }
        if (p.res2) {
            const bf16_t* rz = p.res2 + (mw0_ + (lane_e & 31)) * p.ldr2 + ps * 64 + (lane_e >> 5) * 4;
#pragma unroll
            for (int k = 0; k < 8; ++k) q2[k] = *reinterpret_cast<const u32x2*>(rz + (k >> 2) * 32 + (k & 3) * 8);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) q2[k] = u32x2{0, 0};
        }
    };

    while (true) {
        const long long mw0 = blk * 128 + wave * 32;
        tick(I1{}, I0{}, IX{}, I0{}, I1{}, 0);       // A(1) G(0)            DMA W1(2) W2(1)
        for (int j = 1; j + 2 < nslab; j += 2) {
            tick(I0{}, I1{}, I0{}, I1{}, I1{}, j);   // A(j+1) G(j) B(j-1)   DMA W1(j+2) W2(j+1)
            tick(I1{}, I0{}, I1{}, I0{}, I1{}, j + 1);
        }
        // penultimate tick: no A (its x fragments are dead: fetch the next block's), then the boundary tick A'(0) + B(last)
        const long long nxt = blk + gridDim.x;
        load_x(nxt < nblocks ? nxt : blk);
        tick(IX{}, I1{}, I0{}, I1{}, I0{}, nslab - 1);   // G(last) B(last-1)    DMA W1'(1)
        // <LN>: the block's LayerNorm on the freshly loaded rows (their load latency went under the tick above); ~170 VALU per block
        if constexpr (LN) ln_rows_inplace<NK>(xr, p.ln_eps);
        fetch_res(mw0, 0, r1[0], r2[0]);                   // the epilogue's first pass: in flight under the boundary tick
        tick(I0{}, IX{}, I1{}, IX{}, I1{}, nslab);   // A'(0) B(last)        DMA W2'(0)

        // ---- block epilogue: out = c_acc (acc + b2) + c1 res1 + c2 res2, 32 rows x 64 channels per staging pass
        {
            // the lane ids go through an opaque copy: otherwise every address below is hoisted out of the block loop, ~80 VGPRs that
            // live (spilled) through the ticks and make the scheduler refuse the interleaved tick order as too register-hungry
            int lane_e = lane;
            asm volatile("" : "+v"(lane_e));
            const int l31 = lane_e & 31, hi = lane_e >> 5, lane = lane_e;
            const long long m = mw0 + l31;
            float ca = p.c_acc, c1 = p.c_res1, c2 = p.c_res2;
            if (p.coef) {
                const float* cf = p.coef + (m / p.coef_rpg) * 3;
                ca = cf[0]; c1 = cf[1]; c2 = cf[2];
            }
#pragma unroll
            for (int ps = 0; ps < NO / 2; ++ps) {
                const int col0 = ps * 64;
                if (ps + 1 < NO / 2) fetch_res(mw0, ps + 1, r1[(ps + 1) & 1], r2[(ps + 1) & 1]);   // one pass ahead of its use
                if (p.res1) {                                  // coalesced residual rows -> LDS -> MFMA layout
#pragma unroll
                    for (int it = 0; it < 4; ++it) {
                        const int c = it * 64 + lane;
                        *reinterpret_cast<u32x4*>(stage + (c >> 3) * SROW + (c & 7) * 16) = r1[ps & 1][it];
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
#pragma unroll
                for (int oo = 0; oo < 2; ++oo) {
                    const int o = ps * 2 + oo;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int ch = oo * 32 + g * 8 + hi * 4;          // channel inside the pass
                        const float4 b = *reinterpret_cast<const float4*>(lds + B2_OFF + (col0 + ch) * 4);
                        float v[4] = {ca * (acc2[o][4 * g + 0] + b.x), ca * (acc2[o][4 * g + 1] + b.y), ca * (acc2[o][4 * g + 2] + b.z),
                                      ca * (acc2[o][4 * g + 3] + b.w)};
                        if (p.res1) {
                            const uint2 rr = *reinterpret_cast<const uint2*>(stage + l31 * SROW + ch * 2);
                            v[0] += c1 * bflo(rr.x); v[1] += c1 * bfhi(rr.x); v[2] += c1 * bflo(rr.y); v[3] += c1 * bfhi(rr.y);
                        }
                        if (p.res2) {
                            const u32x2 rr = r2[ps & 1][oo * 4 + g];
                            v[0] += c2 * bflo(rr.x); v[1] += c2 * bfhi(rr.x); v[2] += c2 * bflo(rr.y); v[3] += c2 * bfhi(rr.y);
                        }
                        *reinterpret_cast<uint2*>(stage + l31 * SROW + ch * 2) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc2[o][r] = 0.f;
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                bf16_t* oz = p.out + mw0 * p.ldo + col0;
#pragma unroll
                for (int c0 = 0; c0 < 256; c0 += 64) {
                    const int c = c0 + lane;
                    *reinterpret_cast<uint4*>(oz + (long long)(c >> 3) * p.ldo + (c & 7) * 8) =
                        *reinterpret_cast<const uint4*>(stage + (c >> 3) * SROW + (c & 7) * 16);
                }
            }
        }
        if (nxt >= nblocks) break;
        blk = nxt;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace

static int ff_fused_launch(const void* x, int64_t ldx, float ln_eps, const void* W1p, const float* b1, const void* W2p, const float* b2,
                           const void* res1, int64_t ldr1, const void* res2, int64_t ldr2, const float* coef, int64_t coef_rpg,
                           float c_acc, float c_res1, float c_res2, void* out, int64_t ldo, int64_t M, int32_t C, int32_t hidden,
                           v3d_stream_t stream) {
    V3D_REQUIRE(x && W1p && b1 && W2p && b2 && out, "v3d_ff_fused: null pointer");
    V3D_REQUIRE(C == 320, "v3d_ff_fused: built for C = 320 (got %d); wider levels use the two-GEMM path", C);
    V3D_REQUIRE(hidden >= 128 && hidden % 64 == 0 && hidden * (long long)C * 4 < (1ll << 31), "v3d_ff_fused: bad hidden size %d", hidden);
    V3D_REQUIRE(M > 0 && M % 128 == 0, "v3d_ff_fused: M must be a multiple of 128 (got %lld)", (long long)M);
    V3D_REQUIRE(ldx % 8 == 0 && ldo % 8 == 0 && (!res1 || ldr1 % 8 == 0) && (!res2 || ldr2 % 4 == 0), "v3d_ff_fused: row strides");
    V3D_REQUIRE(((((uintptr_t)x | (uintptr_t)W1p | (uintptr_t)W2p | (uintptr_t)out | (uintptr_t)b1 | (uintptr_t)b2) & 15) == 0) &&
                    (!res1 || ((uintptr_t)res1 & 15) == 0) && (!res2 || ((uintptr_t)res2 & 7) == 0),
                "v3d_ff_fused: misaligned pointer");
    V3D_REQUIRE(!coef || coef_rpg > 0, "v3d_ff_fused: coef_rpg must be > 0");
    FFP p;
    p.x = (const bf16_t*)x; p.W1 = (const bf16_t*)W1p; p.W2 = (const bf16_t*)W2p; p.b1 = b1; p.b2 = b2;
    p.res1 = (const bf16_t*)res1; p.res2 = (const bf16_t*)res2; p.coef = coef; p.out = (bf16_t*)out;
    p.M = M; p.ldx = ldx; p.ldr1 = ldr1; p.ldr2 = ldr2; p.ldo = ldo; p.coef_rpg = coef_rpg;
    p.c_acc = c_acc; p.c_res1 = c_res1; p.c_res2 = c_res2; p.hidden = hidden; p.ln_eps = ln_eps;
    p.w1_bytes = (unsigned)(2ll * hidden * C * 2);
    p.w2_bytes = (unsigned)((long long)C * hidden * 2);
    const long long nblocks = M / 128;
    const int grid = (int)(nblocks < v3d_num_cus() ? nblocks : v3d_num_cus());
    if (ln_eps > 0.f)
        hipLaunchKernelGGL((ff_fused_kernel<320, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL((ff_fused_kernel<320, false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    return v3d_check_launch("v3d_ff_fused");
}

extern "C" int v3d_ff_fused(const void* x, int64_t ldx, const void* W1p, const float* b1, const void* W2p, const float* b2,
                            const void* res1, int64_t ldr1, const void* res2, int64_t ldr2, const float* coef, int64_t coef_rpg,
                            float c_acc, float c_res1, float c_res2, void* out, int64_t ldo, int64_t M, int32_t C, int32_t hidden,
                            v3d_stream_t stream) {
    return ff_fused_launch(x, ldx, 0.f, W1p, b1, W2p, b2, res1, ldr1, res2, ldr2, coef, coef_rpg, c_acc, c_res1, c_res2, out, ldo, M, C, hidden, stream);
}

extern "C" int v3d_ln_ff_fused(const void* x, int64_t ldx, float ln_eps, const void* W1p, const float* b1, const void* W2p, const float* b2,
                               const void* res1, int64_t ldr1, const void* res2, int64_t ldr2, const float* coef, int64_t coef_rpg,
                               float c_acc, float c_res1, float c_res2, void* out, int64_t ldo, int64_t M, int32_t C, int32_t hidden,
                               v3d_stream_t stream) {
    V3D_REQUIRE(ln_eps > 0.f, "v3d_ln_ff_fused: ln_eps must be > 0");
    return ff_fused_launch(x, ldx, ln_eps, W1p, b1, W2p, b2, res1, ldr1, res2, ldr2, coef, coef_rpg, c_acc, c_res1, c_res2, out, ldo, M, C, hidden, stream);
}
