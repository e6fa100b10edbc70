// Patch-stationary packed split kernel for 3x3 / pad 1 / stride 1 convolutions (operand mode 4) on the pre-split weight image.
//
// The packed ring kernel (conv_ring_kernel.h, <1, 4, 1, 0>) splits every activation into its three bf16 planes when the fragment is
// read: once per tap, per wave column and per N tile -- 9 * 2 * Cout / 64 times per input element.  Here one workgroup (256 threads,
// 4 waves) owns a PH x PW patch of output pixels of ONE image (never across an image boundary) and a group of the 32-column blocks of
// N, as conv_astat_kernel.h does for the 1x1 layers:
//   phase 1  the input patch with its one-pixel halo, (PH + 2) x (PW + 2) pixels x Cin, is loaded once (8 threads per pixel and 32-channel
//            step: one 128-byte run, 16 bytes per thread; x_ld is honoured; coordinates clamped into the frame, so nothing outside the
//            tensor is read), split ONCE (sn_split_level / sn_pack_bf16: the arithmetic of sn_split3_pair) and written to LDS
//            pixel-major: per pixel and 16-deep k group 96 bytes = [plane h, m, l][lane half g][8 bf16], element e of half g holds
//            channel 16 q + 8 (e >> 2) + 4 g + (e & 3) -- the k order of the weight image (conv.h).  Halo pixels outside the frame
//            hold zeros: the ring kernel reads a zero page for those taps, so the planes (all zero) are the same bits.  With stride 1
//            every tap of every patch pixel -- also of the pixels of a ragged patch that lie beyond the frame and are never stored --
//            is one of the halo entries, so no separate zero entry is needed.
//   LDS pitch  a 32-row block is 4 x 8 pixels of the patch, lane i its pixel (i >> 3, i & 7).  ds_read_b128 serves a wave in four 16-lane groups
//            ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32), i.e. in a group two rows with pixels 0-3 and two with
//            pixels 4-7; a group is conflict-free when its 16 lanes hit the 16 different 16-byte slots of the 256-byte bank row.
//            No single pitch over a 10-pixel halo row does that, so pixels and rows have pitches of their own:
//              pixel pitch = 6 Cin + 16 bytes: an ODD number of 16-byte slots (6 Cin = 12 slots per 32 channels), so the four
//                            pixels of a row quarter take four different slots, and slots 0..7 mod 8 over a row of 8;
//              row pitch   = 128 (mod 256) bytes (the PW + 2 pixels rounded up): neighbouring rows differ by 8 slots, rows two apart by 0.
//            A group's rows r and r + 3 (the same pixel quarter) are then 8 slots apart, r + 1 and r + 2 likewise, and the two
//            pairs use different quarters: 16 different slots.  A tap only adds a constant.
//   phase 2  wave w works on row unit w % RU (WR 32-row blocks of the patch, RU = RB / WR units) and on the column blocks
//            b, b + 4 / RU, ... of the workgroup's group.  K runs in the ring kernel's MODE 1 order: tap (kh, kw) outer, channels
//            inner in 32-deep steps -- the order of the weight image.  Per 16-deep k group the A planes come from LDS at the lane's
//            pixel shifted by the tap (one running byte offset), the B planes straight from the image in global memory (lane-linear
//            16-byte loads into three rotating register sets, two K steps ahead), then the six MFMAs of the group in the product
//            order and k-group order of the packed ring step, accumulators from zero, K steps ascending.  With WR = 2 a wave
//            multiplies both of its row blocks with one B fragment: half the B traffic per MFMA.
//   K halves  a launch the ring kernel runs as <1, 4, 2, 0> (p.splitk == 2, equal halves: two groups of waves accumulate one half of K
//            each from zero and group 0 adds group 1's parked sums to its own before the epilogue) is reproduced by the wave itself:
//            at the middle of K the accumulators are set aside and cleared, at the end the two halves are added, first + second.
//   epilogue conv_epilogue's arithmetic in its order, with the row -> M map of a 2-D patch (conv_patch_epilogue below).
// Every output element is therefore the same chain of MFMAs and adds as in the ring kernel: the results are bit-identical.
// No LDS-DMA, no pinned registers, no inline-asm waits, nothing shared between workgroups: the compiler's own waits are right.
#pragma once
#include "conv_kernel.h"

#ifndef PATCH_ABLATE
#define PATCH_ABLATE 0         // probe-only bit mask (never set in the library build): 1 no phase-1 global loads, 2 no B loads behind the first
                               // NS - 1, 4 no epilogue stores, 8 no LDS reads of the A planes
#endif

constexpr int sn_patch_pixel_bytes(int cin) { return cin * 6 + 16; }
constexpr int sn_patch_row_bytes(int pw, int cin) { return (((pw + 2) * sn_patch_pixel_bytes(cin) + 127) & ~255) + 128; }
// dynamic LDS of a workgroup: the planes of the halo patch + the four waves' epilogue scratches
constexpr size_t sn_patch_lds_bytes(int ph, int pw, int cin) { return (size_t)(ph + 2) * sn_patch_row_bytes(pw, cin) + 4 * 4096; }

// conv_epilogue<TM, 1> (conv_kernel.h) for row blocks whose 32 rows are 4 x 8 pixels of a patch: mrow[i][q] is the M row of block
// i's rows (lane >> 3) + 8 q, or -1 where the pixel lies beyond the frame (nothing is stored; the residual is read at m_safe).
// The scratch is wave-private LDS; plain accesses: there is no LDS-DMA in flight in this kernel.
template <int TM>
__device__ __forceinline__ void conv_patch_epilogue(f32x16 (&acc)[TM][1], const ConvArgs& p, const int (&mrow)[TM][4], int m_safe, int nw0,
                                                    int lane, float* scratch) {
    const bool has_res = p.residual != nullptr;
    const bool has_obn = p.out_scale != nullptr;
    const bool has_bias = p.bias != nullptr;
    const bool relu = p.relu_out;
    const bool res_plain = p.res_stride == 1 && p.res_H == p.Ho && p.res_W == p.Wo;
    float* const wr = scratch + (4 * (lane >> 5)) * 32 + (lane & 31);                        // C/D role
    const int rrow = lane >> 3, rc4 = (lane & 7) * 4;                                        // row-major role: rows rrow + 8q
    const float* const rd = scratch + rrow * 32 + rc4;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        unsigned roff[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = mrow[i][q] >= 0 ? mrow[i][q] : m_safe;
            if (!has_res || res_plain) {
                roff[q] = (unsigned)(m * p.res_ld);
            } else {
                const int img = sn_fastdiv(m, p.div_hw_mul, p.div_hw_shift);
                const int rr = m - img * (p.Ho * p.Wo);
                const int oy = sn_fastdiv(rr, p.div_w_mul, p.div_w_shift), ox = rr - oy * p.Wo;
                roff[q] = (unsigned)(((img * p.res_H + oy * p.res_stride) * p.res_W + ox * p.res_stride) * p.res_ld);
            }
        }
        const int n = nw0 + rc4;
        const bool ncol = n < p.Cout;
        const int nc = min(n, p.Cout - 4);
        float4 rv[4];
        if (has_res) {
#pragma unroll
            for (int q = 0; q < 4; ++q) rv[q] = *reinterpret_cast<const float4*>(p.residual + (roff[q] + (unsigned)nc));
        }
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 bv = has_bias ? *reinterpret_cast<const float4*>(p.bias + nc) : zero4;
        const float4 os = has_obn ? *reinterpret_cast<const float4*>(p.out_scale + nc) : zero4;
        const float4 ob = has_obn ? *reinterpret_cast<const float4*>(p.out_shift + nc) : zero4;
        const bool has_floor = has_obn && p.out_floor != nullptr;
        const float4 fl = has_floor ? *reinterpret_cast<const float4*>(p.out_floor + nc) : zero4;
#pragma unroll
        for (int r = 0; r < 16; ++r) wr[((r & 3) + 8 * (r >> 2)) * 32] = acc[i][0][r];
        f32x4 t[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = *reinterpret_cast<const f32x4*>(rd + q * 256);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 v = make_float4(t[q].x, t[q].y, t[q].z, t[q].w);
            v.x += bv.x; v.y += bv.y; v.z += bv.z; v.w += bv.w;
            if (has_res) { v.x += rv[q].x; v.y += rv[q].y; v.z += rv[q].z; v.w += rv[q].w; }
            if (has_obn) {
                v.x = __builtin_fmaf(v.x, os.x, ob.x); v.y = __builtin_fmaf(v.y, os.y, ob.y);
                v.z = __builtin_fmaf(v.z, os.z, ob.z); v.w = __builtin_fmaf(v.w, os.w, ob.w);
            }
            if (has_floor) { v.x = fmaxf(v.x, fl.x); v.y = fmaxf(v.y, fl.y); v.z = fmaxf(v.z, fl.z); v.w = fmaxf(v.w, fl.w); }
            else if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            if ((PATCH_ABLATE & 4) ? v.x == 123.456f : true)
            if (ncol && mrow[i][q] >= 0) *reinterpret_cast<float4*>(p.y + ((size_t)mrow[i][q] * p.Cout + n)) = v;
        }
    }
}

template <int PH, int PW /* the patch: PH x PW pixels = RB 32-row blocks of 4 x 8 pixels */, int WR /* row blocks a wave multiplies with one B fragment */,
          int NS /* rotating register sets of B planes: NS - 1 K steps in flight */>
__global__ __launch_bounds__(256, WR >= 4 ? 1 : 2) void conv_patch_f32_kernel(const ConvArgs p) {
    constexpr int HW = PW + 2, NPIX = (PH + 2) * HW, RBX = PW / 8, RB = (PH / 4) * RBX;
    static_assert(PH % 4 == 0 && PW % 8 == 0 && RB % WR == 0 && (RB / WR == 1 || RB / WR == 2) && NS >= 3, "row blocks of 4 x 8 pixels, one or two row units");
    constexpr int RU = RB / WR;                            // row units of the patch: waves w and w + RU share a unit's rows
    constexpr int CS = 4 / RU;                             // column blocks between a wave's consecutive blocks
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) unsigned char patch_lds[];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int csteps = p.Cin >> 5, steps = 9 * csteps;     // 32-deep K steps per tap / in all
    const int PB = sn_patch_pixel_bytes(p.Cin), RPB = sn_patch_row_bytes(PW, p.Cin);
    // (patch, N group) of this workgroup through the XCD remap of the other conv kernels: the patches that share an XCD are one
    // contiguous run (x fastest, then y), so their halos hit in that XCD's L2 and the output lies there as the ring kernel leaves it
    const ConvTile tile = conv_tile_of_block(p);
    const int tiles_x = (p.Wo + PW - 1) / PW, tiles_img = tiles_x * ((p.Ho + PH - 1) / PH);
    const int img = tile.mt / tiles_img, t_in = tile.mt - img * tiles_img;
    const int oy0 = (t_in / tiles_x) * PH, ox0 = (t_in % tiles_x) * PW;
    const int grp = tile.nt;

    // ---- phase 1: 8 threads per (halo pixel, 32-channel step); thread `sub` holds channels 32 cs + 4 sub ..+3, which is k group
    // 2 cs + (sub >> 2), lane half g = sub & 1, elements 4 ((sub >> 1) & 1) ..+3 of that half's entry
    {
        const int sub = tid & 7;
        const unsigned ent = (unsigned)((sub >> 2) * 96 + (sub & 1) * 16 + ((sub >> 1) & 1) * 8);
        const int nitems = NPIX * csteps;
        constexpr int U = NPIX > 150 ? 8 : 4;
        // U items in flight; an item index beyond the last is clamped to it (the same values written to the same place again) so
        // that the loads are unconditional and stay ahead of the splits
        for (int it0 = tid >> 3; it0 < nitems; it0 += 32 * U) {
            f32x4 v[U];
            unsigned dst[U];
            bool in[U];
#pragma unroll
            for (int i = 0; i < U; ++i) {
                const int it = min(it0 + 32 * i, nitems - 1);
                const int hp = it / csteps, cs = it - hp * csteps;
                const int hy = hp / HW, hx = hp - hy * HW;
                const int iy = oy0 - 1 + hy, ix = ox0 - 1 + hx;
                in[i] = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
                const int iyc = min(max(iy, 0), p.H - 1), ixc = min(max(ix, 0), p.W - 1);
                if (!(PATCH_ABLATE & 1)) v[i] = *reinterpret_cast<const f32x4*>(p.x + (size_t)((img * p.H + iyc) * p.W + ixc) * p.x_ld + (cs * 32 + sub * 4));
                else v[i] = f32x4{(float)iyc, (float)ixc, (float)sub, 1.f};
                dst[i] = (unsigned)(hy * RPB + hx * PB + cs * 192) + ent;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < U; ++i) {
                float a = in[i] ? v[i].x : 0.f, b = in[i] ? v[i].y : 0.f, c = in[i] ? v[i].z : 0.f, d = in[i] ? v[i].w : 0.f;
                u32x2 h, m, l;
                h.x = sn_split_level(a, b); h.y = sn_split_level(c, d);
                m.x = sn_split_level(a, b); m.y = sn_split_level(c, d);
                l.x = sn_pack_bf16(a, b); l.y = sn_pack_bf16(c, d);
                *reinterpret_cast<u32x2*>(patch_lds + dst[i]) = h;
                *reinterpret_cast<u32x2*>(patch_lds + dst[i] + 32) = m;
                *reinterpret_cast<u32x2*>(patch_lds + dst[i] + 64) = l;
            }
        }
    }
    __syncthreads();

    // ---- phase 2: this wave's row unit and its column blocks b, b + CS, ... of the workgroup's group (a multiple of CS blocks)
    const int nblk = 2 * ((p.Cout + 63) >> 6);
    const int bpg = (((nblk + (int)gridDim.y - 1) / (int)gridDim.y) + CS - 1) / CS * CS;
    const int b_end = min(min(nblk, (grp + 1) * bpg), (p.Cout + 31) >> 5);    // (the image is zero beyond Cout: skipped)
    const int ru = wave % RU;
    int b = grp * bpg + wave / RU;
    if (b >= b_end) return;
    float* const scratch = reinterpret_cast<float*>(patch_lds + (PH + 2) * RPB + wave * SN_EPI_WAVE_BYTES);
    // block i of the unit is row block ru WR + i of the patch: 4 x 8 pixels at (4 by, 8 bx).  The M rows of the epilogue's row-major
    // role: rows (lane >> 3) + 8 q of the block = patch pixel (4 by + q, 8 bx + (lane >> 3))
    int mrow[WR][4];
    unsigned blk_off[WR];
#pragma unroll
    for (int i = 0; i < WR; ++i) {
        const int by = (ru * WR + i) / RBX, bx = (ru * WR + i) % RBX;
        blk_off[i] = (unsigned)(4 * by * RPB + 8 * bx * PB);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int oy = oy0 + 4 * by + q, ox = ox0 + 8 * bx + (lane >> 3);
            mrow[i][q] = (oy < p.Ho && ox < p.Wo) ? (img * p.Ho + oy) * p.Wo + ox : -1;
        }
    }
    const int m_safe = (img * p.Ho + oy0) * p.Wo + ox0;
    // image, in 16-byte units: (N tile, K step) 768 = [wave column 2][plane 3][k group 2][lane 64]
    const f32x4* lp = reinterpret_cast<const f32x4*>(p.w) + ((size_t)(b >> 1) * steps * 12 + (b & 1) * 6) * 64 + lane;
    // the lane's pixel (C/D column role: row lane & 31 of the block = patch pixel (lane & 31) >> 3, lane & 7) at tap (0, 0), half g
    const unsigned char* const abase = patch_lds + (unsigned)(((lane & 31) >> 3) * RPB + (lane & 7) * PB + (lane >> 5) * 16);
    // The wave's work is one stream of items (column block, K step), NS rotating register sets of B planes as in conv_astat_kernel.h:
    // item i is multiplied from set i % NS while items i + 1 .. i + NS - 1 are in flight.  The loads are unconditional: behind the last
    // item the loader stays where it is and fetches that item again.
    const int items = ((b_end - b + CS - 1) / CS) * steps;
    const int adv_block = 768 * ((CS / 2 - 1) * steps + 1);    // last K step of a block -> first of the wave's next (CS / 2 N tiles on)
    int l_item = 0, l_ks = 0;
    auto load = [&](f32x4 (&dst)[6]) {
        if ((PATCH_ABLATE & 2) && l_item >= NS - 1) return;
#pragma unroll
        for (int i = 0; i < 6; ++i) dst[i] = lp[i * 64];
        const int adv = l_item + 1 >= items ? 0 : (l_ks + 1 < steps ? 768 : adv_block);
        lp += adv;
        ++l_item;
        l_ks = l_ks + 1 < steps ? l_ks + 1 : 0;
        __builtin_amdgcn_sched_barrier(0);                  // (the scheduler would sink the loads to their first use)
    };
    f32x16 acc[WR][1], first_half[WR];
    const int half = p.splitk == 2 ? steps >> 1 : steps;   // the K step at which the second accumulator set begins (none: steps)
#pragma unroll
    for (int i = 0; i < WR; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) first_half[i][e] = 0.f;
    auto zero = [&]() {
#pragma unroll
        for (int i = 0; i < WR; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][0][e] = 0.f;
    };
    // K position: step ks = tap (kh, kw) x channel step cs; a_off = the tap's pixel shift + the channel step's planes, in bytes
    int ks = 0, cs = 0, kw = 0;
    unsigned a_off = 0;
    auto item = [&](const f32x4 (&B)[6]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            SnPlanes A[WR];
#pragma unroll
            for (int i = 0; i < WR; ++i) {
                const unsigned char* ap = abase + (a_off + (unsigned)(j * 96) + blk_off[i]);
                if (!(PATCH_ABLATE & 8)) {
                    A[i].h = *reinterpret_cast<const sn_u32x4*>(ap);
                    A[i].m = *reinterpret_cast<const sn_u32x4*>(ap + 32);
                    A[i].l = *reinterpret_cast<const sn_u32x4*>(ap + 64);
                } else {
                    A[i].h = A[i].m = A[i].l = sn_u32x4{(unsigned)(size_t)ap, a_off, (unsigned)lane, 1u};
                }
            }
            // the six products of sn_mfma_split3_pk in its order, the row blocks' independent accumulators taking turns: every
            // accumulator sees its own chain unchanged, and no MFMA waits for the one issued just before it
            const sn_bf16x8 bh = __builtin_bit_cast(sn_bf16x8, B[j]), bm = __builtin_bit_cast(sn_bf16x8, B[2 + j]), bl = __builtin_bit_cast(sn_bf16x8, B[4 + j]);
#define SN_PATCH_MFMA(ap_, b_)                                                                                                      \
    _Pragma("unroll") for (int i = 0; i < WR; ++i)                                                                                  \
        acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(sn_bf16x8, A[i].ap_), b_, acc[i][0], 0, 0, 0)
            SN_PATCH_MFMA(l, bh);
            SN_PATCH_MFMA(h, bl);
            SN_PATCH_MFMA(m, bm);
            SN_PATCH_MFMA(m, bh);
            SN_PATCH_MFMA(h, bm);
            SN_PATCH_MFMA(h, bh);
#undef SN_PATCH_MFMA
        }
        a_off += 192;
        if (++cs == csteps) {                               // next tap: the next pixel, or the first pixel of the next halo row
            cs = 0;
            a_off += 16;                                    // (csteps * 192 = 6 Cin = the pixel pitch - 16)
            if (++kw == 3) { kw = 0; a_off += (unsigned)(RPB - 3 * PB); }
        }
        if (++ks == half && half != steps) {
#pragma unroll
            for (int i = 0; i < WR; ++i) first_half[i] = acc[i][0];
            zero();
        }
        if (ks == steps) {
            if (half != steps) {
#pragma unroll
                for (int i = 0; i < WR; ++i)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[i][0][e] = first_half[i][e] + acc[i][0][e];
            }
            conv_patch_epilogue<WR>(acc, p, mrow, m_safe, b * 32, lane, scratch);
            b += CS;
            ks = 0;
            a_off = 0;
            zero();
        }
    };
    f32x4 B[NS][6];
    zero();
#pragma unroll
    for (int s = 0; s < NS - 1; ++s) load(B[s]);
    for (int it = 0; it < items; it += NS) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (it + s >= items) break;
            load(B[(s + NS - 1) % NS]);
            item(B[s]);
        }
    }
}
