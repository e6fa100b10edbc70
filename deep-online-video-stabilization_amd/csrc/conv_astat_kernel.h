// A-stationary packed split kernel for wide, shallow 1x1 convolutions (K <= 256, no K split) on the pre-split weight image.
//
// The packed ring kernel (conv_ring_kernel.h, <0, 4, 1, 0>) splits every activation into its three bf16 planes when the fragment is
// read, once per 32-column wave tile: 2 * Cout / 64 times per element (16 times at Cout = 512, 32 times at 1024), and that VALU work
// -- not the matrix pipe -- bounds its K step.  Here one workgroup (256 threads, 4 waves) owns BM rows of M and a group of the
// 32-column blocks of N:
//   phase 1  the A tile [BM][K] is loaded once (coalesced 16-byte loads, rows clamped to M - 1), split ONCE (sn_split_level /
//            sn_pack_bf16: the arithmetic of sn_split3_pair) and written to LDS fragment-major: per 32-row block and 16-deep k group
//            [plane h, m, l][lane 64][8 bf16], lane = row + 32 g, element e holds k = 16 q + 8 (e >> 2) + 4 g + (e & 3) -- the k order
//            of the weight image (conv.h);
//   phase 2  every wave loops over its column blocks: block 2 t + wn is (N tile t, wave column wn) of the weight image.  Per k group
//            the A planes come from LDS (ds_read_b128), the B planes straight from the image in global memory into registers
//            (lane-linear 16-byte loads, two 32-deep K steps ahead; no wave shares a B fragment with another), then the six MFMAs of
//            the group in the product order and k-group order of the packed ring step, accumulators from zero, K steps ascending;
//   epilogue conv_epilogue<BM / 32, 1> on a wave-private scratch.
// Workgroup ids go through conv_tile_of_block() (XCD remap) like the other conv kernels'.
// Every output element is therefore the same chain of MFMAs as in the ring kernel: the results are bit-identical.
// No LDS-DMA, no cross-tile pipelining, nothing shared between workgroups: the compiler's own waits are right.
#pragma once
#include "conv_kernel.h"

constexpr int SN_ASTAT_A_BYTES = 48 * 1024;       // BM * K * 6: BM = 32 up to K = 256

template <int BM>
__global__ __launch_bounds__(256, 2) void conv_astat_f32_kernel(const ConvArgs p) {
    // BM = 32 is the one instantiation conv.hip builds and launches.  The body is written for one or two 32-row blocks: the 64-row
    // form (K <= 128) was instantiated once for the measurement recorded in DESIGN.md section 4, round 10, and measured level.
    static_assert(BM == 32 || BM == 64, "one or two 32-row blocks");
    constexpr int RB = BM / 32;
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    __shared__ __attribute__((aligned(16))) unsigned char lds[SN_ASTAT_A_BYTES + 4 * SN_EPI_WAVE_BYTES];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int steps = p.K >> 5, kq = 2 * steps;            // 32-deep K steps, 16-deep k groups
    // (M tile, N group) of this workgroup: the XCD remap of the other conv kernels (conv_tile_of_block: the ids that share an XCD get
    // one contiguous run of M tiles, the groups of an M tile next to each other), so the output lies in the L2s as the ring kernel
    // leaves it for the next launch
    const ConvTile tile = conv_tile_of_block(p);
    const int m0 = tile.mt * BM, grp = tile.nt;

    // ---- phase 1: 8 threads per (row, K step) = one 128-byte run; thread `sub` holds k = 32 ks + 4 sub ..+3, which is k group
    // 2 ks + (sub >> 2), lane half g = sub & 1, elements 4 ((sub >> 1) & 1) ..+3 of the lane's entry
    {
        const int r = tid >> 3, sub = tid & 7;
        const unsigned ent = (unsigned)((r + 32 * (sub & 1)) * 16 + 8 * ((sub >> 1) & 1));
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const int row = min(m0 + rb * 32 + r, p.M - 1);
            const float* src = p.x + (size_t)row * p.x_ld + sub * 4;
            // four K steps in flight; a step index beyond the last is clamped to it (the same values written to the same place
            // again) so that nothing here is conditional and the loads stay ahead of the splits
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
    __syncthreads();

    // ---- phase 2: this wave's column blocks b, b + 4, ... of the workgroup's group (a multiple of four blocks per group)
    const int nblk = 2 * ((p.Cout + 63) >> 6);
    const int bpg = (((nblk + (int)gridDim.y - 1) / (int)gridDim.y) + 3) & ~3;
    const int b_end = min(min(nblk, (grp + 1) * bpg), (p.Cout + 31) >> 5);    // (the image is zero beyond Cout: skipped)
    int b = grp * bpg + wave;
    if (b >= b_end) return;
    const unsigned scratch = (unsigned)(size_t)(__attribute__((address_space(3))) void*)lds + (unsigned)(SN_ASTAT_A_BYTES + wave * SN_EPI_WAVE_BYTES);
    // image, in 16-byte units: (N tile, K step) 768 = [wave column 2][plane 3][k group 2][lane 64]
    const f32x4* lp = reinterpret_cast<const f32x4*>(p.w) + ((size_t)(b >> 1) * steps * 12 + (b & 1) * 6) * 64 + lane;
    const unsigned char* afrag = lds + lane * 16;
    // The wave's work is one stream of items (column block, K step).  Three register sets of B planes ([plane][k group] of one K
    // step, 24 registers each) rotate through it: item i is multiplied from set i % 3 while items i + 1 and i + 2 are in flight --
    // two K steps of MFMAs cover the L2 latency, across the epilogues as well.  The loads are unconditional: behind the last item
    // the loader stays where it is and fetches that item again.
    const int items = ((b_end - b + 3) >> 2) * steps;
    int l_item = 0, l_ks = 0;
    auto load = [&](f32x4 (&dst)[6]) {
#pragma unroll
        for (int i = 0; i < 6; ++i) dst[i] = lp[i * 64];
        // on to the next K step of the block, or to the first of the wave's next block (two N tiles on)
        const int adv = l_item + 1 >= items ? 0 : (l_ks + 1 < steps ? 768 : 768 * (steps + 1));
        lp += adv;
        ++l_item;
        l_ks = l_ks + 1 < steps ? l_ks + 1 : 0;
        __builtin_amdgcn_sched_barrier(0);                  // (the scheduler would sink the loads to their first use)
    };
    f32x16 acc[RB][1];
    auto zero = [&]() {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[rb][0][e] = 0.f;
    };
    int ks = 0;
    auto item = [&](const f32x4 (&B)[6]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const unsigned char* ap = afrag + (unsigned)((rb * kq + 2 * ks + j) * 3072);
                SnPlanes A;
                A.h = *reinterpret_cast<const sn_u32x4*>(ap);
                A.m = *reinterpret_cast<const sn_u32x4*>(ap + 1024);
                A.l = *reinterpret_cast<const sn_u32x4*>(ap + 2048);
                sn_mfma_split3_pk(acc[rb][0], A, B[j], B[2 + j], B[4 + j]);
            }
        }
        if (++ks == steps) {
            conv_epilogue<RB, 1>(acc, p, m0, b * 32, lane, 0, scratch);
            b += 4;
            ks = 0;
            zero();
        }
    };
    f32x4 B0[6], B1[6], B2[6];
    zero();
    load(B0);
    load(B1);
    for (int it = 0; it < items; it += 3) {
        load(B2); item(B0);
        if (it + 1 >= items) break;
        load(B0); item(B1);
        if (it + 2 >= items) break;
        load(B1); item(B2);
    }
}
