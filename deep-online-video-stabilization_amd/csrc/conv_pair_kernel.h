// A bottleneck unit's 1x1 `conv3` (+ bias + residual) and the NEXT identity unit's 1x1 `conv1` (pre-activation BN + ReLU prologue, consumer
// BN + ReLU epilogue) as ONE launch.  conv3's output is the next residual and is written as before; what goes is conv1's pass over it: every
// element conv1 reads was in a conv3 accumulator one launch earlier.
//
// One workgroup (256 threads, 4 waves) owns BM rows of M and does the whole pair for them:
//   phase 1  the A tile [BM][K1] of conv3, once:
//              packed form (F32A = 0)  split into bf16 planes, fragment-major, exactly as conv_astat_kernel.h phase 1 lays it out;
//              f32 form (F32A = 1, K1 = 64: the launches conv_route() keeps on the exact-f32 register-staged kernel)  plain floats,
//              [row][16 x 16 bytes], the 16-byte column index XOR (row & 15) so that the fragment reads of 16 rows hit 16 bank groups;
//   per pass of 128 output channels of conv3 (wave w: the 32-column block 4 pass + w, every 32-row block of the tile):
//     phase A  packed: the B planes from conv3's weight image into two alternating register sets (one 32-deep K step ahead),
//              sn_mfma_split3_pk with k groups ascending -- the chain of conv_astat_f32_kernel / conv_ring_f32_kernel<0, 4, 1, 0>;
//              f32: the weights [Cout][64] straight from memory, v_mfma_f32_32x32x2_f32 with the k order of conv_igemm_body.h (lane half h
//              takes k = 8 kk + 4 h + e, kk and e ascending);
//              then conv_epilogue's arithmetic through a scratch (the 6 KB of the chunk this wave is about to write: the scratch is back in
//              registers before the first of those writes): (acc + bias) + residual, stored raw, 16 bytes per lane; the
//              same registers get max(fma(v, scale[c], shift[c]), 0) with the next unit's pre-activation vectors (SN_PRO of the ring
//              kernel), are split (sn_split_level / sn_pack_bf16) and written to the LDS chunk [32-row block][k group 8][plane 3][lane 64]
//              [8 bf16] -- the astat fragment layout with k = channel;
//     barrier
//     phase B  every wave multiplies the chunk with its 32-column block of conv1's weight image (k groups 8 pass .. 8 pass + 7: K2 = N1
//              ascending from zeroed accumulators that live across the passes -- the chain of conv_ring_f32_kernel<0, 4, 1, 1> without
//              a K split);
//     barrier  (the chunk is free for the next pass)
//   epilogue conv_epilogue<1, 1> with conv1's arguments (its consumer BN + ReLU).
// BM = 64 with two column blocks of conv1 (N2 = 64: 2 x 2 wave tiles), BM = 32 with four (N2 = 128).  LDS = A tile + one chunk (24 KB per
// 32-row block): 48 KB (BM 32, K1 128: three workgroups per CU), 64 KB (BM 64, K1 64, f32: two).
// Plain loads, stores and __syncthreads() only; nothing is shared between workgroups.  Workgroup ids go through conv_tile_of_block().
#pragma once
#include "conv_kernel.h"

struct ConvUnitPairArgs { ConvArgs a /* conv3; a.w = its weight image (packed form) or its weights (f32 form) */, b /* conv1; b.w = its weight image */; };

constexpr int SN_PAIR_PASS = 128;                    // output channels of conv3 per pass: four 32-column blocks, one per wave
// LDS: the A tile + the chunk of a pass, per 32-row block SN_PAIR_PASS / 16 k groups of [plane 3][lane 64][16 bytes]
static inline size_t sn_pair_a_bytes(int f32a, int bm, int k1) { return f32a ? (size_t)bm * 256 : (size_t)bm * k1 * 6; }
static inline size_t sn_pair_lds_bytes(int f32a, int bm, int k1) { return sn_pair_a_bytes(f32a, bm, k1) + (size_t)(bm / 32) * (SN_PAIR_PASS / 16) * 3072; }

// conv3's epilogue for one 32-column block of the wave (conv_epilogue's arithmetic for bias + plain residual, no consumer BN), and the
// pre-activated, split copy of the same values into the chunk (cl0 = the block's first channel inside the 128-channel pass).
// The transposition scratch of row block i is the 6 KB of the chunk that this wave alone writes for it (k groups cl0 / 16 and the next of
// row block i): the scratch is in registers before the first of those writes.
template <int RB, int CHUNK_RB>
__device__ __forceinline__ void conv_pair_epilogue_a(f32x16 (&acc)[RB], const ConvArgs& p, const float* pre_scale, const float* pre_shift, int m0, int n0,
                                                     int cl0, int lane, unsigned chunk_lds, unsigned char* chunk) {
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    const bool has_res = p.residual != nullptr, has_bias = p.bias != nullptr;
    const int rrow = lane >> 3, rc4 = (lane & 7) * 4;                                        // row-major role: rows rrow + 8q
    const int n = n0 + rc4, cl = cl0 + rc4;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 bv = has_bias ? *reinterpret_cast<const float4*>(p.bias + n) : zero4;
    const float4 ps = *reinterpret_cast<const float4*>(pre_scale + n), pb = *reinterpret_cast<const float4*>(pre_shift + n);
    // the lane's four channels are k = 16 (cl >> 4) + 8 half + 4 g + 0..3 of the chunk: elements 4 half ..+3 of entry (row + 32 g)
    unsigned char* const cdst = chunk + (unsigned)((cl >> 4) * 3072 + 32 * ((cl >> 2) & 1) * 16 + 8 * ((cl >> 3) & 1));
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        int mrow[4];
        float4 rv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            mrow[q] = m0 + i * 32 + rrow + 8 * q;
            if (has_res) rv[q] = *reinterpret_cast<const float4*>(p.residual + ((unsigned)(min(mrow[q], p.M - 1) * p.res_ld) + (unsigned)n));
        }
        const unsigned scratch = chunk_lds + (unsigned)(i * CHUNK_RB + (cl0 >> 4) * 3072);
        const unsigned wr = scratch + (unsigned)(((4 * (lane >> 5)) * 32 + (lane & 31)) * 4);   // C/D role
        const unsigned rd = scratch + (unsigned)((rrow * 32 + rc4) * 4);
        {
            const f32x16 a = acc[i];
            SN_EPI_W(0); SN_EPI_W(1); SN_EPI_W(2); SN_EPI_W(3); SN_EPI_W(4); SN_EPI_W(5); SN_EPI_W(6); SN_EPI_W(7);
            SN_EPI_W(8); SN_EPI_W(9); SN_EPI_W(10); SN_EPI_W(11); SN_EPI_W(12); SN_EPI_W(13); SN_EPI_W(14); SN_EPI_W(15);
        }
        f32x4 t[4];
        SN_EPI_R(0, t[0]); SN_EPI_R(1, t[1]); SN_EPI_R(2, t[2]); SN_EPI_R(3, t[3]);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3])::"memory");
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 v = make_float4(t[q].x, t[q].y, t[q].z, t[q].w);
            v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
            if (has_res) { v.x += rv[q].x; v.y += rv[q].y; v.z += rv[q].z; v.w += rv[q].w; }
            if (mrow[q] < p.M) *reinterpret_cast<float4*>(p.y + ((size_t)mrow[q] * p.Cout + n)) = v;
            float a = fmaxf(__builtin_fmaf(v.x, ps.x, pb.x), 0.f), b = fmaxf(__builtin_fmaf(v.y, ps.y, pb.y), 0.f);
            float c = fmaxf(__builtin_fmaf(v.z, ps.z, pb.z), 0.f), d = fmaxf(__builtin_fmaf(v.w, ps.w, pb.w), 0.f);
            u32x2 h, m, l;
            h.x = sn_split_level(a, b); h.y = sn_split_level(c, d);
            m.x = sn_split_level(a, b); m.y = sn_split_level(c, d);
            l.x = sn_pack_bf16(a, b); l.y = sn_pack_bf16(c, d);
            unsigned char* dst = cdst + (unsigned)(i * CHUNK_RB + (rrow + 8 * q) * 16);
            *reinterpret_cast<u32x2*>(dst) = h;
            *reinterpret_cast<u32x2*>(dst + 1024) = m;
            *reinterpret_cast<u32x2*>(dst + 2048) = l;
        }
    }
}

template <int F32A, int BM>
__global__ __launch_bounds__(256, 2) void conv_unit_pair_f32_kernel(const ConvUnitPairArgs P) {
    static_assert(BM == 32 || BM == 64, "one or two 32-row blocks");
    constexpr int PW = SN_PAIR_PASS;
    constexpr int RB = BM / 32;
    constexpr int CBW = PW / 32;                           // column blocks of a pass
    constexpr int RBW = RB * CBW / 4;                      // row blocks a wave takes in phase A
    constexpr int SB = PW / 32;                            // K steps of conv1 per pass
    constexpr int CHUNK_RB = (PW / 16) * 3072;
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const ConvArgs& p = P.a;
    const ConvArgs& c1 = P.b;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int steps = p.K >> 5, kq = 2 * steps;           // conv3: 32-deep K steps, 16-deep k groups
    const int steps2 = p.Cout >> 5;                        // conv1: K2 = conv3's Cout
    const int passes = p.Cout / PW;
    const ConvTile tile = conv_tile_of_block(p);
    const int m0 = tile.mt * BM;
    const unsigned a_bytes = F32A ? (unsigned)(BM * 256) : (unsigned)(BM * p.K * 6);
    unsigned char* const chunk = lds + a_bytes;
    const unsigned chunk_lds = (unsigned)(size_t)(__attribute__((address_space(3))) void*)lds + a_bytes;
    // phase A: this wave's column block of a pass and its first row block
    const int cbA = wave % CBW, rbA0 = (wave / CBW) * RBW;

    // ---- phase 1
    if constexpr (F32A) {
        const int r = tid >> 4, c = tid & 15;             // 16 threads per row of 64 floats
        f32x4 v[BM / 16];
#pragma unroll
        for (int i = 0; i < BM / 16; ++i) v[i] = *reinterpret_cast<const f32x4*>(p.x + (size_t)min(m0 + r + 16 * i, p.M - 1) * p.x_ld + 4 * c);
#pragma unroll
        for (int i = 0; i < BM / 16; ++i) *reinterpret_cast<f32x4*>(lds + (unsigned)((r + 16 * i) * 256 + ((c ^ (r & 15)) * 16))) = v[i];
    } else {
        // (conv_astat_kernel.h phase 1)
        const int r = tid >> 3, sub = tid & 7;
        const unsigned ent = (unsigned)((r + 32 * (sub & 1)) * 16 + 8 * ((sub >> 1) & 1));
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const float* src = p.x + (size_t)min(m0 + rb * 32 + r, p.M - 1) * p.x_ld + sub * 4;
            for (int ks0 = 0; ks0 < steps; ks0 += 4) {
                f32x4 v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const f32x4*>(src + 32 * min(ks0 + i, steps - 1));
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float a = v[i].x, b = v[i].y, c = v[i].z, d = v[i].w;
                    u32x2 h, m, l;
                    h.x = sn_split_level(a, b); h.y = sn_split_level(c, d);
                    m.x = sn_split_level(a, b); m.y = sn_split_level(c, d);
                    l.x = sn_pack_bf16(a, b); l.y = sn_pack_bf16(c, d);
                    unsigned char* dst = lds + (unsigned)((rb * kq + 2 * min(ks0 + i, steps - 1) + (sub >> 2)) * 3072) + ent;
                    *reinterpret_cast<u32x2*>(dst) = h;
                    *reinterpret_cast<u32x2*>(dst + 1024) = m;
                    *reinterpret_cast<u32x2*>(dst + 2048) = l;
                }
            }
        }
    }

    // conv1: this wave's (32-row block, 32-column block) and its column block's planes in the image, 16-byte units:
    // (N tile, K step) 768 = [wave column 2][plane 3][k group 2][lane 64]
    const int rb2 = RB == 2 ? (wave >> 1) : 0, cb2 = RB == 2 ? (wave & 1) : wave;
    const f32x4* const w1p = reinterpret_cast<const f32x4*>(c1.w) + ((size_t)(cb2 >> 1) * steps2 * 12 + (cb2 & 1) * 6) * 64 + lane;
    f32x4 C0[6], C1[6];
    auto load2 = [&](f32x4 (&dst)[6], int ks2) {
        const f32x4* lp = w1p + (size_t)min(ks2, steps2 - 1) * 768;
#pragma unroll
        for (int i = 0; i < 6; ++i) dst[i] = lp[i * 64];
        __builtin_amdgcn_sched_barrier(0);                  // (the scheduler would sink the loads to their first use)
    };
    f32x16 acc2[1][1];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc2[0][0][e] = 0.f;
    const unsigned char* const cfrag = chunk + (unsigned)(rb2 * CHUNK_RB + lane * 16);
    auto step2 = [&](const f32x4 (&B)[6], int s) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned char* ap = cfrag + (unsigned)((2 * s + j) * 3072);
            SnPlanes A;
            A.h = *reinterpret_cast<const sn_u32x4*>(ap);
            A.m = *reinterpret_cast<const sn_u32x4*>(ap + 1024);
            A.l = *reinterpret_cast<const sn_u32x4*>(ap + 2048);
            sn_mfma_split3_pk(acc2[0][0], A, B[j], B[2 + j], B[4 + j]);
        }
    };

    // conv3, packed form: block b = 4 pass + wave of the image; f32 form: weight row n = 128 pass + 32 wave + (lane & 31), k = 8 kk + 4 h ..+3
    const f32x4* const w3p = F32A ? reinterpret_cast<const f32x4*>(p.w + (size_t)(32 * cbA + (lane & 31)) * p.K + 4 * (lane >> 5))
                                  : reinterpret_cast<const f32x4*>(p.w) + ((size_t)(cbA >> 1) * steps * 12 + (cbA & 1) * 6) * 64 + lane;
    f32x4 W3[8];                                           // f32 form: the wave's weights of a pass
    f32x4 S0[6], S1[6];                                    // packed form: B planes of two K steps
    auto load3 = [&](f32x4 (&dst)[6], int pass, int ks) {     // packed: (pass, K step) of this wave's column block (CBW / 2 N tiles per pass)
        const f32x4* lp = w3p + ((size_t)((CBW / 2) * min(pass, passes - 1)) * steps + min(ks, steps - 1)) * 768;
#pragma unroll
        for (int i = 0; i < 6; ++i) dst[i] = lp[i * 64];
        __builtin_amdgcn_sched_barrier(0);
    };
    auto load3f = [&](f32x4 (&dst)[8], int pass) {            // f32: the 64 k of this wave's rows of the pass
        const f32x4* lp = w3p + (size_t)(PW * min(pass, passes - 1)) * (p.K >> 2);
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) dst[kk] = lp[2 * kk];
        __builtin_amdgcn_sched_barrier(0);
    };
    f32x16 acc[RBW];
    const unsigned char* const afrag = lds + lane * 16;
    auto step3 = [&](const f32x4 (&B)[6], int ks) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int rb = 0; rb < RBW; ++rb) {
                const unsigned char* ap = afrag + (unsigned)(((rbA0 + rb) * kq + 2 * ks + j) * 3072);
                SnPlanes A;
                A.h = *reinterpret_cast<const sn_u32x4*>(ap);
                A.m = *reinterpret_cast<const sn_u32x4*>(ap + 1024);
                A.l = *reinterpret_cast<const sn_u32x4*>(ap + 2048);
                sn_mfma_split3_pk(acc[rb], A, B[j], B[2 + j], B[4 + j]);
            }
        }
    };

    if constexpr (F32A) load3f(W3, 0);
    else load3(S0, 0, 0);
    load2(C0, 0);
    __syncthreads();

    for (int pass = 0; pass < passes; ++pass) {
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[rb][e] = 0.f;
        // ---- phase A
        if constexpr (F32A) {
            const int arow = lane & 31, h = lane >> 5;
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) {
#pragma unroll
                for (int rb = 0; rb < RBW; ++rb) {
                    const f32x4 af = *reinterpret_cast<const f32x4*>(lds + (unsigned)(((rbA0 + rb) * 32 + arow) * 256 + (((2 * kk + h) ^ (arow & 15)) * 16)));
                    acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, W3[kk].x, acc[rb], 0, 0, 0);
                    acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, W3[kk].y, acc[rb], 0, 0, 0);
                    acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, W3[kk].z, acc[rb], 0, 0, 0);
                    acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, W3[kk].w, acc[rb], 0, 0, 0);
                }
            }
            load3f(W3, pass + 1);                           // the next pass's weights fly under the epilogue and phase B
        } else {
            for (int ks = 0; ks < steps; ks += 2) {        // (K1 is a multiple of 64)
                load3(S1, pass, ks + 1);
                step3(S0, ks);
                if (ks + 2 < steps) load3(S0, pass, ks + 2);
                else load3(S0, pass + 1, 0);                // ... the next pass's first step flies under the epilogue and phase B
                step3(S1, ks + 1);
            }
        }
        conv_pair_epilogue_a<RBW, CHUNK_RB>(acc, p, c1.in_scale, c1.in_shift, m0 + 32 * rbA0, PW * pass + 32 * cbA, 32 * cbA, lane,
                                            chunk_lds + (unsigned)(rbA0 * CHUNK_RB), chunk + rbA0 * CHUNK_RB);
        __syncthreads();
        // ---- phase B: K steps SB pass .. SB pass + SB - 1 of conv1
#pragma unroll
        for (int s = 0; s < SB; s += 2) {
            load2(C1, SB * pass + s + 1);
            step2(C0, s);
            load2(C0, SB * pass + s + 2);                   // (s + 2 == SB: the next pass's first step; behind the last: that step again, unused)
            step2(C1, s + 1);
        }
        __syncthreads();
    }
    // (the chunk is free: the wave's own 6 KB of it as the scratch)
    conv_epilogue<1, 1>(acc2, c1, m0 + rb2 * 32, cb2 * 32, lane, 0, chunk_lds + (unsigned)(rbA0 * CHUNK_RB + 2 * cbA * 3072));
}
