// Baseline JPEG (JFIF, SOF0, 8-bit, Huffman) encoder for the stabilised frames, gfx950: the frame is already in device memory
// (stabnet_warp_rev_bundle2 / stabnet_cvt_train2img), so it is compressed there and only the compressed bytes cross PCIe.
// One frame = four launches, no host synchronisation, allocation or copy (capturable in a hipGraph with the frame):
//   mjpeg_transform_kernel : BGR/grey -> float32 YCbCr (JFIF full range, no 8-bit rounding), 2x2 chroma mean (4:2:0), level
//                            shift, 8x8 orthonormal DCT-II (row pass, column pass through LDS), rint(coef / Q), clamp, zig-zag;
//                            int16 coefficients in SCAN order: [mcu][block of the MCU][64]
//   mjpeg_entropy_kernel   : one lane per restart interval (DC predictors start at 0 there, so intervals are independent):
//                            Annex K Huffman codes, byte stuffing, 1-bit padding -> the interval's slot, its length beside it
//   mjpeg_layout_kernel    : exclusive scan of (length + 2) over the intervals of a frame, header copy, out_bytes
//   mjpeg_gather_kernel    : one wave per interval: slot -> its place in the stream, RSTm after it (EOI after the last)
// Every buffer is sized for the worst case of a block (an 11-bit DC difference and 63 AC values of 16 + 10 bits < 208 bytes,
// every byte stuffed: 416 bytes), so nothing can be written past a slot or past stabnet_mjpeg_max_bytes.
#include "common.h"
#include "jpeg_tables.h"
#include "prof.h"

namespace {

enum { MJ_GREY = 0, MJ_444 = 1, MJ_420 = 2 };
constexpr int kBlockWorstBytes = 416;

struct MjGeom {
    int mode, ms, bpm, mcux, mcuy, nmcu, nint, ncomp;
    size_t nblk, slot_bytes;
};

bool mj_geom(int H, int W, int C, int subsampling, int restart_mcus, MjGeom* g) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || (C != 1 && C != 3)) return false;
    if (C == 3 && subsampling != 420 && subsampling != 444) return false;
    if (restart_mcus < 1 || restart_mcus > 65535) return false;
    g->mode = C == 1 ? MJ_GREY : (subsampling == 420 ? MJ_420 : MJ_444);
    g->ms = g->mode == MJ_420 ? 16 : 8;
    g->bpm = g->mode == MJ_420 ? 6 : (g->mode == MJ_444 ? 3 : 1);
    g->ncomp = C;
    g->mcux = (W + g->ms - 1) / g->ms;
    g->mcuy = (H + g->ms - 1) / g->ms;
    g->nmcu = g->mcux * g->mcuy;
    g->nint = (g->nmcu + restart_mcus - 1) / restart_mcus;
    g->nblk = (size_t)g->nmcu * g->bpm;
    g->slot_bytes = (size_t)restart_mcus * g->bpm * kBlockWorstBytes;
    if (g->nmcu < restart_mcus) g->slot_bytes = (size_t)g->nmcu * g->bpm * kBlockWorstBytes;
    return true;
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// SOI 2, APP0 18, DQT 4 + 65 per table, SOF0 10 + 3 C, DHT 4 + (17 + 12 + 17 + 162) per table pair, DRI 6, SOS 8 + 2 C
int mj_header_size(int C) {
    const int ntab = C == 1 ? 1 : 2;
    return 2 + 18 + 4 + 65 * ntab + 10 + 3 * C + 4 + ntab * 208 + 6 + 8 + 2 * C;
}

// per-frame workspace: coefficients | interval lengths | interval offsets | interval slots
struct MjWs { size_t coef, lens, offs, slots, frame; };
MjWs mj_ws(const MjGeom& g) {
    MjWs w;
    w.coef = 0;
    w.lens = align16(g.nblk * 64 * sizeof(short));
    w.offs = w.lens + align16((size_t)g.nint * sizeof(int));
    w.slots = w.offs + align16((size_t)g.nint * sizeof(int));
    w.frame = w.slots + align16((size_t)g.nint * g.slot_bytes);
    return w;
}

// ---- tables of the standard (ITU-T T.81 Annex K) ------------------------------------------------------------------------------
constexpr unsigned char kQLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                      14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                      18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr unsigned char kQChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                        99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// What the kernels read: the DCT matrix, natural -> zig-zag positions, and the Huffman code of every symbol as (code << 8) | length
// (Annex C: codes of one length are consecutive, the first of a length is twice the one after the last of the previous length).
struct MjTables {
    float dct[8][8];               // dct[u][x] = c(u)/2 * cos((2x+1) u pi/16)
    unsigned char zzpos[64];       // natural index -> position in the scan
    unsigned dc[2][12];            // [luma|chroma][category]
    unsigned ac[2][256];           // [luma|chroma][run << 4 | size]; 0 = no such symbol
};

constexpr MjTables make_tables() {
    MjTables t{};
    // 0.5 * cos(k pi/16), k = 0..8
    const double hc[9] = {0.5, 0.49039264020161522, 0.46193976625564337, 0.41573480615127262, 0.35355339059327379,
                          0.27778511650980114, 0.19134171618254492, 0.09754516100806417, 0.0};
    for (int u = 0; u < 8; ++u)
        for (int x = 0; x < 8; ++x) {
            double v = 0.0;
            if (u == 0) {
                v = 0.35355339059327379;
            } else {
                const int k = ((2 * x + 1) * u) % 32;
                v = k <= 8 ? hc[k] : (k <= 16 ? -hc[16 - k] : (k < 24 ? -hc[k - 16] : hc[32 - k]));
            }
            t.dct[u][x] = (float)v;
        }
    for (int z = 0; z < 64; ++z) t.zzpos[kZigzag[z]] = (unsigned char)z;
    for (int tab = 0; tab < 2; ++tab) {
        unsigned code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kDcBits[tab][len - 1]; ++i) t.dc[tab][kDcVals[k++]] = (code++ << 8) | (unsigned)len;
            code <<= 1;
        }
        code = 0; k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kAcBits[tab][len - 1]; ++i) t.ac[tab][kAcVals[tab][k++]] = (code++ << 8) | (unsigned)len;
            code <<= 1;
        }
    }
    return t;
}

__constant__ const MjTables d_tab = make_tables();

// ---- transform -----------------------------------------------------------------------------------------------------------------
// One wave = one group of consecutive MCUs that fills 6 or 8 blocks: 4:2:0 one MCU (Y00 Y01 Y10 Y11 Cb Cr), 4:4:4 two MCUs
// (Y Cb Cr each), grey eight MCUs.  Blocks sit in LDS at a stride of 72 floats, so that the column pass (lane = block, column)
// touches 64 different banks.  No FMA contraction (-ffp-contract=off): the sums are plain float32 in index order.
constexpr int kBlkStride = 72;

template <int MODE>
__global__ __launch_bounds__(256) void mjpeg_transform_kernel(const unsigned char* __restrict__ img, int H, int W, int mcux, int nmcu,
                                                              const unsigned short* __restrict__ qluma,
                                                              const unsigned short* __restrict__ qchroma, short* __restrict__ coef,
                                                              size_t coef_frame_stride) {
    constexpr int MPW = MODE == MJ_420 ? 1 : (MODE == MJ_444 ? 2 : 8);     // MCUs per wave
    constexpr int BPM = MODE == MJ_420 ? 6 : (MODE == MJ_444 ? 3 : 1);     // blocks per MCU
    constexpr int NB = MPW * BPM;
    constexpr int C = MODE == MJ_GREY ? 1 : 3;
    __shared__ __attribute__((aligned(16))) float s_blk[4][8 * kBlkStride];
    __shared__ __attribute__((aligned(16))) short s_out[4][8 * 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.y;
    const int m0 = (blockIdx.x * 4 + wave) * MPW;
    const unsigned char* im = img + (size_t)n * H * W * C;
    float* blk = s_blk[wave];
    short* outb = s_out[wave];

    if (m0 < nmcu) {
        if (MODE == MJ_420) {
            const int my = m0 / mcux, mx = m0 - my * mcux;
            const int qy = lane >> 3, qx = lane & 7;
            float cb = 0.f, cr = 0.f;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int py = 2 * qy + (d >> 1), px = 2 * qx + (d & 1);
                const int y = min(my * 16 + py, H - 1), x = min(mx * 16 + px, W - 1);     // partial MCUs replicate the edge
                const unsigned char* p = im + ((size_t)y * W + x) * 3;
                const float B = (float)p[0], G = (float)p[1], R = (float)p[2];
                blk[((py >> 3) * 2 + (px >> 3)) * kBlkStride + (py & 7) * 8 + (px & 7)] = 0.299f * R + 0.587f * G + 0.114f * B - 128.0f;
                cb += -0.168735892f * R - 0.331264108f * G + 0.5f * B;
                cr += 0.5f * R - 0.418687589f * G - 0.081312411f * B;
            }
            blk[4 * kBlkStride + lane] = cb * 0.25f;
            blk[5 * kBlkStride + lane] = cr * 0.25f;
        } else {
#pragma unroll
            for (int j = 0; j < MPW; ++j) {
                const int m = min(m0 + j, nmcu - 1);                  // past the last MCU: a copy that is never stored
                const int my = m / mcux, mx = m - my * mcux;
                const int y = min(my * 8 + (lane >> 3), H - 1), x = min(mx * 8 + (lane & 7), W - 1);
                const unsigned char* p = im + ((size_t)y * W + x) * C;
                if (MODE == MJ_GREY) {
                    blk[j * kBlkStride + lane] = (float)p[0] - 128.0f;
                } else {
                    const float B = (float)p[0], G = (float)p[1], R = (float)p[2];
                    blk[(j * 3 + 0) * kBlkStride + lane] = 0.299f * R + 0.587f * G + 0.114f * B - 128.0f;
                    blk[(j * 3 + 1) * kBlkStride + lane] = -0.168735892f * R - 0.331264108f * G + 0.5f * B;
                    blk[(j * 3 + 2) * kBlkStride + lane] = 0.5f * R - 0.418687589f * G - 0.081312411f * B;
                }
            }
        }
    }
    __syncthreads();
    const int b = lane >> 3, r = lane & 7;
    if (m0 < nmcu && lane < NB * 8) {               // rows: lane = (block, row)
        float* row = blk + b * kBlkStride + r * 8;
        float in[8], o[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) in[x] = row[x];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float s = d_tab.dct[u][0] * in[0];
#pragma unroll
            for (int x = 1; x < 8; ++x) s += d_tab.dct[u][x] * in[x];
            o[u] = s;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) row[u] = o[u];
    }
    __syncthreads();
    if (m0 < nmcu && lane < NB * 8) {               // columns: lane = (block, column); quantise, clamp, zig-zag
        const float* col = blk + b * kBlkStride + r;
        const bool luma = MODE == MJ_GREY ? true : (MODE == MJ_444 ? (b % 3 == 0) : (b < 4));
        const unsigned short* q = luma ? qluma : qchroma;
        float in[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = col[k * 8];
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            float s = d_tab.dct[v][0] * in[0];
#pragma unroll
            for (int k = 1; k < 8; ++k) s += d_tab.dct[v][k] * in[k];
            const int nat = v * 8 + r;
            float t = rintf(s / (float)q[nat]);
            const float lim = nat == 0 ? 1024.0f : 1023.0f;           // every value keeps a baseline Huffman category
            t = fminf(fmaxf(t, -lim), lim);
            outb[b * 64 + d_tab.zzpos[nat]] = (short)(int)t;
        }
    }
    __syncthreads();
    if (m0 < nmcu) {
        const int nvb = min(MPW, nmcu - m0) * BPM;                    // blocks of MCUs that exist
        unsigned* dst = reinterpret_cast<unsigned*>(coef + (size_t)n * coef_frame_stride + (size_t)m0 * BPM * 64);
        const unsigned* src = reinterpret_cast<const unsigned*>(outb);
        for (int i = lane; i < nvb * 32; i += 64) dst[i] = src[i];
    }
}

// The same transform from a planar frame (stabnet_mjpeg_encode_i420): Y [H,W] and, for MJ_420, Cb and Cr [H/2,W/2] behind it, dense,
// frames frame_stride bytes apart.  The samples ARE the JFIF components, so the load stage is a level shift: no colour arithmetic and no
// 2x2 mean.  4:2:0: a lane loads four luma samples of one row of the 16x16 patch (a dword where it is aligned and inside the row) and
// one sample each of Cb and Cr; partial MCUs replicate the edge sample of the plane.  From the first barrier on these are the lines of
// mjpeg_transform_kernel, repeated here and not shared: that kernel's code must not move (tools/isa_hash.py).
template <int MODE>
__global__ __launch_bounds__(256) void mjpeg_transform_planar_kernel(const unsigned char* __restrict__ src, size_t frame_stride, int H, int W,
                                                                     int mcux, int nmcu, const unsigned short* __restrict__ qluma,
                                                                     const unsigned short* __restrict__ qchroma, short* __restrict__ coef,
                                                                     size_t coef_frame_stride) {
    static_assert(MODE == MJ_420 || MODE == MJ_GREY, "planar frames are 4:2:0 or grey");
    constexpr int MPW = MODE == MJ_420 ? 1 : 8;                            // MCUs per wave
    constexpr int BPM = MODE == MJ_420 ? 6 : 1;                            // blocks per MCU
    constexpr int NB = MPW * BPM;
    __shared__ __attribute__((aligned(16))) float s_blk[4][8 * kBlkStride];
    __shared__ __attribute__((aligned(16))) short s_out[4][8 * 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = blockIdx.y;
    const int m0 = (blockIdx.x * 4 + wave) * MPW;
    const unsigned char* im = src + (size_t)n * frame_stride;
    float* blk = s_blk[wave];
    short* outb = s_out[wave];

    if (m0 < nmcu) {
        if (MODE == MJ_420) {
            const int my = m0 / mcux, mx = m0 - my * mcux;
            {
                const int py = lane >> 2, px = (lane & 3) * 4;            // four samples of row py of the patch
                const int y = min(my * 16 + py, H - 1), x = mx * 16 + px;
                const unsigned char* row = im + (size_t)y * W;
                unsigned v;
                if (x + 4 <= W && ((uintptr_t)(row + x) & 3) == 0) {
                    v = *reinterpret_cast<const unsigned*>(row + x);
                } else {
                    v = 0u;
#pragma unroll
                    for (int k = 0; k < 4; ++k) v |= (unsigned)row[min(x + k, W - 1)] << (8 * k);
                }
                float* d = blk + ((py >> 3) * 2 + (px >> 3)) * kBlkStride + (py & 7) * 8 + (px & 7);
#pragma unroll
                for (int k = 0; k < 4; ++k) d[k] = (float)((v >> (8 * k)) & 0xffu) - 128.0f;
            }
            const int CH = H >> 1, CW = W >> 1;
            const int cy = min(my * 8 + (lane >> 3), CH - 1), cx = min(mx * 8 + (lane & 7), CW - 1);
            const unsigned char* cb = im + (size_t)H * W;
            const unsigned char* cr = cb + (size_t)CH * CW;
            blk[4 * kBlkStride + lane] = (float)cb[(size_t)cy * CW + cx] - 128.0f;
            blk[5 * kBlkStride + lane] = (float)cr[(size_t)cy * CW + cx] - 128.0f;
        } else {
#pragma unroll
            for (int j = 0; j < MPW; ++j) {
                const int m = min(m0 + j, nmcu - 1);                  // past the last MCU: a copy that is never stored
                const int my = m / mcux, mx = m - my * mcux;
                const int y = min(my * 8 + (lane >> 3), H - 1), x = min(mx * 8 + (lane & 7), W - 1);
                blk[j * kBlkStride + lane] = (float)im[(size_t)y * W + x] - 128.0f;
            }
        }
    }
    __syncthreads();
    const int b = lane >> 3, r = lane & 7;
    if (m0 < nmcu && lane < NB * 8) {               // rows: lane = (block, row)
        float* row = blk + b * kBlkStride + r * 8;
        float in[8], o[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) in[x] = row[x];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float s = d_tab.dct[u][0] * in[0];
#pragma unroll
            for (int x = 1; x < 8; ++x) s += d_tab.dct[u][x] * in[x];
            o[u] = s;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) row[u] = o[u];
    }
    __syncthreads();
    if (m0 < nmcu && lane < NB * 8) {               // columns: lane = (block, column); quantise, clamp, zig-zag
        const float* col = blk + b * kBlkStride + r;
        const bool luma = MODE == MJ_GREY ? true : (b < 4);
        const unsigned short* q = luma ? qluma : qchroma;
        float in[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) in[k] = col[k * 8];
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            float s = d_tab.dct[v][0] * in[0];
#pragma unroll
            for (int k = 1; k < 8; ++k) s += d_tab.dct[v][k] * in[k];
            const int nat = v * 8 + r;
            float t = rintf(s / (float)q[nat]);
            const float lim = nat == 0 ? 1024.0f : 1023.0f;           // every value keeps a baseline Huffman category
            t = fminf(fmaxf(t, -lim), lim);
            outb[b * 64 + d_tab.zzpos[nat]] = (short)(int)t;
        }
    }
    __syncthreads();
    if (m0 < nmcu) {
        const int nvb = min(MPW, nmcu - m0) * BPM;                    // blocks of MCUs that exist
        unsigned* dst = reinterpret_cast<unsigned*>(coef + (size_t)n * coef_frame_stride + (size_t)m0 * BPM * 64);
        const unsigned* srcw = reinterpret_cast<const unsigned*>(outb);
        for (int i = lane; i < nvb * 32; i += 64) dst[i] = srcw[i];
    }
}

// ---- entropy coding ------------------------------------------------------------------------------------------------------------
struct BitSink {
    unsigned char* out;
    unsigned long long acc;
    int nb, pos;
    __device__ __forceinline__ void put(unsigned bits, int len) {       // len <= 26, nb < 8 on entry
        acc = (acc << len) | bits;
        nb += len;
        while (nb >= 8) {
            const unsigned byte = (unsigned)(acc >> (nb - 8)) & 0xffu;
            out[pos++] = (unsigned char)byte;
            if (byte == 0xffu) out[pos++] = 0;
            nb -= 8;
        }
    }
};

template <int MODE>
__global__ __launch_bounds__(256) void mjpeg_entropy_kernel(const short* __restrict__ coef, size_t coef_frame_stride, int nmcu, int R,
                                                            int nint, unsigned char* __restrict__ slots, size_t slot_bytes,
                                                            int* __restrict__ lens, size_t ws_frame_bytes) {
    constexpr int BPM = MODE == MJ_420 ? 6 : (MODE == MJ_444 ? 3 : 1);
    __shared__ unsigned s_ac[2][256];
    __shared__ unsigned s_dc[2][12];
    for (int i = threadIdx.x; i < 512; i += 256) s_ac[i >> 8][i & 255] = d_tab.ac[i >> 8][i & 255];
    if (threadIdx.x < 24) s_dc[threadIdx.x / 12][threadIdx.x % 12] = d_tab.dc[threadIdx.x / 12][threadIdx.x % 12];
    __syncthreads();
    const int it = blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y;
    if (it >= nint) return;
    const short* cf = coef + (size_t)n * coef_frame_stride;
    BitSink s;
    s.out = slots + (size_t)n * ws_frame_bytes + (size_t)it * slot_bytes;
    s.acc = 0ull; s.nb = 0; s.pos = 0;
    int pred0 = 0, pred1 = 0, pred2 = 0;
    const int m_end = min(nmcu, (it + 1) * R);
    for (int m = it * R; m < m_end; ++m) {
        for (int j = 0; j < BPM; ++j) {
            const int comp = MODE == MJ_GREY ? 0 : (MODE == MJ_444 ? j : (j < 4 ? 0 : j - 3));
            const int tab = comp ? 1 : 0;
            const short* blk = cf + ((size_t)m * BPM + j) * 64;
            const uint4* b4 = reinterpret_cast<const uint4*>(blk);
            unsigned long long mask = 0ull;                          // bit k: coefficient k of the scan is not zero
            int dc = 0;
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                const uint4 w = b4[v];
                if (v == 0) dc = (int)(short)(w.x & 0xffffu);
                const unsigned ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (ws[e] & 0xffffu) mask |= 1ull << (v * 8 + e * 2);
                    if (ws[e] >> 16) mask |= 1ull << (v * 8 + e * 2 + 1);
                }
            }
            const int pred = comp == 0 ? pred0 : (comp == 1 ? pred1 : pred2);
            const int diff = dc - pred;
            if (comp == 0) pred0 = dc; else if (comp == 1) pred1 = dc; else pred2 = dc;
            {
                const int a = diff < 0 ? -diff : diff;
                const int size = 32 - __clz(a);                      // 0 for a == 0
                const unsigned h = s_dc[tab][size];
                const unsigned vb = (unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << size) - 1u);
                s.put(((h >> 8) << size) | vb, (int)(h & 0xffu) + size);
            }
            mask &= ~1ull;
            int prev = 0;
            while (mask) {
                const int k = __ffsll((long long)mask) - 1;
                mask &= mask - 1ull;
                int run = k - prev - 1;
                prev = k;
                while (run >= 16) {
                    const unsigned z = s_ac[tab][0xf0];
                    s.put(z >> 8, (int)(z & 0xffu));
                    run -= 16;
                }
                const int v = (int)blk[k];
                const int a = v < 0 ? -v : v;
                const int size = 32 - __clz(a);
                const unsigned h = s_ac[tab][(run << 4) | size];
                const unsigned vb = (unsigned)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
                s.put(((h >> 8) << size) | vb, (int)(h & 0xffu) + size);
            }
            if (prev != 63) {
                const unsigned e = s_ac[tab][0];
                s.put(e >> 8, (int)(e & 0xffu));
            }
        }
    }
    if (s.nb > 0) s.put((1u << (8 - s.nb)) - 1u, 8 - s.nb);          // pad the last byte with 1-bits
    lens[(size_t)n * (ws_frame_bytes / sizeof(int)) + it] = s.pos;
}

// ---- layout: where every interval goes; header; total length ----------------------------------------------------------------------
// One workgroup per frame.  offs[i] = header_bytes + sum_{j<i} (len[j] + 2): every interval is followed by two marker bytes, RSTm
// or, after the last one, EOI -- so the running sum past the last interval is the length of the whole stream.
__global__ __launch_bounds__(1024) void mjpeg_layout_kernel(const int* __restrict__ lens, int* __restrict__ offs, size_t ws_frame_ints,
                                                            int nint, const unsigned char* __restrict__ header, int header_bytes,
                                                            unsigned char* __restrict__ out, size_t out_stride, int* __restrict__ out_bytes) {
    __shared__ int s_wave[16];
    __shared__ int s_carry;
    const int n = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* ln = lens + (size_t)n * ws_frame_ints;
    int* of = offs + (size_t)n * ws_frame_ints;
    unsigned char* o = out + (size_t)n * out_stride;
    for (int i = tid; i < header_bytes; i += 1024) o[i] = header[i];
    if (tid == 0) s_carry = header_bytes;
    __syncthreads();
    for (int base = 0; base < nint; base += 1024) {
        const int i = base + tid;
        const int v = i < nint ? ln[i] + 2 : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = s_carry;
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        if (i < nint) of[i] = before + incl - v;
        __syncthreads();
        if (tid == 1023) s_carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) out_bytes[n] = s_carry;
}

// One wave per interval: the slot's bytes to their place, then RSTm (m counts mod 8) or EOI.
__global__ __launch_bounds__(256) void mjpeg_gather_kernel(const unsigned char* __restrict__ slots, size_t slot_bytes, const int* __restrict__ lens,
                                                           const int* __restrict__ offs, size_t ws_frame_bytes, int nint,
                                                           unsigned char* __restrict__ out, size_t out_stride) {
    const int it = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int n = blockIdx.y;
    if (it >= nint) return;
    const size_t fi = (size_t)n * (ws_frame_bytes / sizeof(int)) + it;
    const int len = lens[fi];
    const unsigned char* src = slots + (size_t)n * ws_frame_bytes + (size_t)it * slot_bytes;
    unsigned char* dst = out + (size_t)n * out_stride + offs[fi];
    for (int i = lane; i < len; i += 64) dst[i] = src[i];
    if (lane == 0) {
        dst[len] = 0xff;
        dst[len + 1] = it == nint - 1 ? (unsigned char)0xd9 : (unsigned char)(0xd0 + (it & 7));
    }
}

// The launches behind the transform (entropy, layout, gather), for stabnet_mjpeg_encode and stabnet_mjpeg_encode_i420 alike.  Defined
// behind stabnet_mjpeg_encode and in front of stabnet_mjpeg_encode_i420: kernels are emitted in the order of their first use, and
// tools/isa_hash.py shows the existing ones unchanged that way.
int mj_launch_tail(const MjGeom& g, const MjWs& w, int N, int restart_mcus, unsigned char* wsb, const unsigned char* header_dev, int header_bytes,
                   unsigned char* out, size_t out_stride, int* out_bytes, hipStream_t st, Prof* prof);

struct ByteOut {
    unsigned char* p;
    int cap, n;
    void u8(int v) { if (p && n < cap) p[n] = (unsigned char)v; ++n; }
    void u16(int v) { u8(v >> 8); u8(v & 0xff); }
};

}  // namespace

extern "C" {

/* Annex K quantisation tables scaled by the IJG rule; natural (row-major) order. */
int stabnet_jpeg_quant_tables(int quality, unsigned short* luma64, unsigned short* chroma64) {
    SN_REQUIRE(luma64 && chroma64, "jpeg_quant_tables: null pointer");
    SN_REQUIRE(quality >= 1 && quality <= 100, "jpeg_quant_tables: quality must be 1..100");
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int l = (kQLuma[i] * s + 50) / 100, c = (kQChroma[i] * s + 50) / 100;
        luma64[i] = (unsigned short)(l < 1 ? 1 : (l > 255 ? 255 : l));
        chroma64[i] = (unsigned short)(c < 1 ? 1 : (c > 255 ? 255 : c));
    }
    return STABNET_OK;
}

/* SOI, APP0 (JFIF 1.01), DQT, SOF0, DHT (the Annex K tables), DRI, SOS: everything before the entropy-coded data.  Returns the
 * number of bytes (host_out may be NULL to ask for it), -1 on bad arguments or when `cap` is too small. */
int stabnet_mjpeg_header(int H, int W, int C, int subsampling, int restart_mcus, const unsigned short* luma64,
                         const unsigned short* chroma64, unsigned char* host_out, int cap) {
    MjGeom g;
    SN_REQUIRE(mj_geom(H, W, C, subsampling, restart_mcus, &g), "mjpeg_header: bad shape, channels, subsampling or restart interval");
    SN_REQUIRE(luma64 && (C == 1 || chroma64), "mjpeg_header: null table");
    for (int i = 0; i < 64; ++i)
        SN_REQUIRE(luma64[i] >= 1 && luma64[i] <= 255 && (C == 1 || (chroma64[i] >= 1 && chroma64[i] <= 255)),
                   "mjpeg_header: baseline quantiser values are 1..255");
    ByteOut o{host_out, host_out ? cap : 0, 0};
    o.u16(0xffd8);
    o.u16(0xffe0); o.u16(16); o.u8('J'); o.u8('F'); o.u8('I'); o.u8('F'); o.u8(0); o.u16(0x0101); o.u8(0); o.u16(1); o.u16(1); o.u8(0); o.u8(0);
    const int ntab = C == 1 ? 1 : 2;
    o.u16(0xffdb); o.u16(2 + 65 * ntab);
    for (int t = 0; t < ntab; ++t) {
        o.u8(t);
        for (int z = 0; z < 64; ++z) o.u8((t ? chroma64 : luma64)[kZigzag[z]]);
    }
    o.u16(0xffc0); o.u16(8 + 3 * C); o.u8(8); o.u16(H); o.u16(W); o.u8(C);
    for (int c = 0; c < C; ++c) { o.u8(c + 1); o.u8(c == 0 && g.mode == MJ_420 ? 0x22 : 0x11); o.u8(c ? 1 : 0); }
    o.u16(0xffc4); o.u16(2 + ntab * (17 + 12 + 17 + 162));
    for (int t = 0; t < ntab; ++t) {
        o.u8(0x00 | t);
        for (int i = 0; i < 16; ++i) o.u8(kDcBits[t][i]);
        for (int i = 0; i < 12; ++i) o.u8(kDcVals[i]);
        o.u8(0x10 | t);
        for (int i = 0; i < 16; ++i) o.u8(kAcBits[t][i]);
        for (int i = 0; i < 162; ++i) o.u8(kAcVals[t][i]);
    }
    o.u16(0xffdd); o.u16(4); o.u16(restart_mcus);
    o.u16(0xffda); o.u16(6 + 2 * C); o.u8(C);
    for (int c = 0; c < C; ++c) { o.u8(c + 1); o.u8(c ? 0x11 : 0x00); }
    o.u8(0); o.u8(63); o.u8(0);
    SN_REQUIRE(!host_out || o.n <= cap, "mjpeg_header: %d bytes needed, cap is %d", o.n, cap);
    return o.n;
}

/* Bytes the caller must provide per frame (out_stride): header + every block at its worst case + markers.  0 on bad arguments. */
size_t stabnet_mjpeg_max_bytes(int H, int W, int C, int subsampling, int restart_mcus) {
    MjGeom g;
    if (!mj_geom(H, W, C, subsampling, restart_mcus, &g)) {
        stabnet_set_error("mjpeg_max_bytes: bad shape, channels, subsampling or restart interval");
        return 0;
    }
    return align16((size_t)mj_header_size(C) + g.nblk * kBlockWorstBytes + 2 * (size_t)g.nint);
}

size_t stabnet_mjpeg_workspace_bytes(int N, int H, int W, int C, int subsampling, int restart_mcus) {
    MjGeom g;
    if (N < 1 || !mj_geom(H, W, C, subsampling, restart_mcus, &g)) {
        stabnet_set_error("mjpeg_workspace_bytes: bad batch, shape, channels, subsampling or restart interval");
        return 0;
    }
    return (size_t)N * mj_ws(g).frame;
}

/* img uint8 [N,H,W,C] (C = 3: BGR; C = 1: grey) -> N JFIF streams at out + n * out_stride, their lengths in out_bytes[n].
 * luma64_dev / chroma64_dev: the quantisation tables in natural order, in device memory (chroma may be NULL when C = 1);
 * header_dev: what stabnet_mjpeg_header wrote for the same arguments, copied to the device by the caller. */
int stabnet_mjpeg_encode(const unsigned char* img, int N, int H, int W, int C, int subsampling, int restart_mcus,
                         const unsigned short* luma64_dev, const unsigned short* chroma64_dev, const unsigned char* header_dev,
                         int header_bytes, unsigned char* out, size_t out_stride, int* out_bytes, void* workspace,
                         size_t workspace_bytes, void* stream, void* profp) {
    SN_REQUIRE(img && luma64_dev && header_dev && out && out_bytes && workspace, "mjpeg_encode: null pointer");
    SN_REQUIRE(C == 1 || C == 3, "mjpeg_encode: C must be 1 (grey) or 3 (BGR), got %d", C);
    SN_REQUIRE(C == 1 || chroma64_dev, "mjpeg_encode: null pointer (chroma table)");
    MjGeom g;
    SN_REQUIRE(N >= 1 && N <= 65535 && mj_geom(H, W, C, subsampling, restart_mcus, &g),
               "mjpeg_encode: bad batch, shape, subsampling (420 | 444) or restart interval (1..65535)");
    const size_t need_out = stabnet_mjpeg_max_bytes(H, W, C, subsampling, restart_mcus);
    SN_REQUIRE(header_bytes == mj_header_size(C), "mjpeg_encode: header_bytes %d, stabnet_mjpeg_header writes %d for C = %d", header_bytes,
               mj_header_size(C), C);
    SN_REQUIRE(out_stride >= need_out, "mjpeg_encode: out_stride %zu < stabnet_mjpeg_max_bytes %zu", out_stride, need_out);
    const MjWs w = mj_ws(g);
    if (workspace_bytes < (size_t)N * w.frame) {
        stabnet_set_error("mjpeg_encode: workspace %zu < %zu bytes", workspace_bytes, (size_t)N * w.frame);
        return STABNET_ERR_WORKSPACE;
    }
    SN_REQUIRE(((uintptr_t)workspace & 15) == 0, "mjpeg_encode: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int rc = sn_check_device(img, "mjpeg_encode: img", st);
    if (rc == 0) rc = sn_check_device(out, "mjpeg_encode: out", st);
    if (rc == 0) rc = sn_check_device(workspace, "mjpeg_encode: workspace", st);
    if (rc) return rc;
    Prof* prof = static_cast<Prof*>(profp);
    unsigned char* wsb = static_cast<unsigned char*>(workspace);
    short* coef = reinterpret_cast<short*>(wsb + w.coef);
    const size_t coef_stride = w.frame / sizeof(short);
    const double px = (double)N * H * W, coef_bytes = (double)N * g.nblk * 128.0;

    const bool rec = prof && prof->begin(st);
    {
        const int mpw = g.mode == MJ_420 ? 1 : (g.mode == MJ_444 ? 2 : 8);
        const dim3 grid(cdiv(cdiv(g.nmcu, mpw), 4), N);
        if (g.mode == MJ_420)
            mjpeg_transform_kernel<MJ_420><<<grid, 256, 0, st>>>(img, H, W, g.mcux, g.nmcu, luma64_dev, chroma64_dev, coef, coef_stride);
        else if (g.mode == MJ_444)
            mjpeg_transform_kernel<MJ_444><<<grid, 256, 0, st>>>(img, H, W, g.mcux, g.nmcu, luma64_dev, chroma64_dev, coef, coef_stride);
        else
            mjpeg_transform_kernel<MJ_GREY><<<grid, 256, 0, st>>>(img, H, W, g.mcux, g.nmcu, luma64_dev, luma64_dev, coef, coef_stride);
    }
    if (rec) prof->end(st, PK_KERNEL_MJPEG_TRANSFORM, 2.0 * 16.0 * (double)N * g.nblk * 64.0, px * C + coef_bytes);
    SN_LAUNCH_CHECK("mjpeg_transform_kernel");

    return mj_launch_tail(g, w, N, restart_mcus, wsb, header_dev, header_bytes, out, out_stride, out_bytes, st, prof);
}

}  // extern "C"

namespace {

int mj_launch_tail(const MjGeom& g, const MjWs& w, int N, int restart_mcus, unsigned char* wsb, const unsigned char* header_dev, int header_bytes,
                   unsigned char* out, size_t out_stride, int* out_bytes, hipStream_t st, Prof* prof) {
    const short* coef = reinterpret_cast<const short*>(wsb + w.coef);
    int* lens = reinterpret_cast<int*>(wsb + w.lens);
    int* offs = reinterpret_cast<int*>(wsb + w.offs);
    unsigned char* slots = wsb + w.slots;
    const size_t coef_stride = w.frame / sizeof(short);
    const double coef_bytes = (double)N * g.nblk * 128.0;

    bool rec = prof && prof->begin(st);
    {
        const dim3 grid(cdiv(g.nint, 256), N);
        if (g.mode == MJ_420)
            mjpeg_entropy_kernel<MJ_420><<<grid, 256, 0, st>>>(coef, coef_stride, g.nmcu, restart_mcus, g.nint, slots, g.slot_bytes, lens, w.frame);
        else if (g.mode == MJ_444)
            mjpeg_entropy_kernel<MJ_444><<<grid, 256, 0, st>>>(coef, coef_stride, g.nmcu, restart_mcus, g.nint, slots, g.slot_bytes, lens, w.frame);
        else
            mjpeg_entropy_kernel<MJ_GREY><<<grid, 256, 0, st>>>(coef, coef_stride, g.nmcu, restart_mcus, g.nint, slots, g.slot_bytes, lens, w.frame);
    }
    if (rec) prof->end(st, PK_KERNEL_MJPEG_ENTROPY, 0.0, coef_bytes);      // + the compressed bytes, known only on the device
    SN_LAUNCH_CHECK("mjpeg_entropy_kernel");

    rec = prof && prof->begin(st);
    mjpeg_layout_kernel<<<N, 1024, 0, st>>>(lens, offs, w.frame / sizeof(int), g.nint, header_dev, header_bytes, out, out_stride, out_bytes);
    if (rec) prof->end(st, PK_KERNEL_MJPEG_LAYOUT, 0.0, (double)N * (8.0 * g.nint + 2.0 * header_bytes));
    SN_LAUNCH_CHECK("mjpeg_layout_kernel");

    rec = prof && prof->begin(st);
    mjpeg_gather_kernel<<<dim3(cdiv(g.nint, 4), N), 256, 0, st>>>(slots, g.slot_bytes, lens, offs, w.frame, g.nint, out, out_stride);
    if (rec) prof->end(st, PK_KERNEL_MJPEG_GATHER, 0.0, (double)N * 8.0 * g.nint);         // + twice the compressed bytes
    SN_LAUNCH_CHECK("mjpeg_gather_kernel");
    return STABNET_OK;
}

}  // namespace

extern "C" {

/* src: N planar frames frame_stride_bytes apart, each Y [H,W] and, for planes = 3, U [H/2,W/2] and V [H/2,W/2] behind it, dense (what
 * stabnet_warp_rev_bundle2_i420 writes) -> the streams of stabnet_mjpeg_encode for C = planes, subsampling 420: header, tables,
 * stabnet_mjpeg_max_bytes and the workspace are those. */
int stabnet_mjpeg_encode_i420(const unsigned char* src, int N, int H, int W, int planes, size_t frame_stride_bytes, int restart_mcus,
                              const unsigned short* luma64_dev, const unsigned short* chroma64_dev, const unsigned char* header_dev,
                              int header_bytes, unsigned char* out, size_t out_stride, int* out_bytes, void* workspace,
                              size_t workspace_bytes, void* stream, void* profp) {
    SN_REQUIRE(src && luma64_dev && header_dev && out && out_bytes && workspace, "mjpeg_encode_i420: null pointer");
    SN_REQUIRE(planes == 1 || planes == 3, "mjpeg_encode_i420: planes must be 1 (Y) or 3 (Y, U, V of 4:2:0), got %d", planes);
    SN_REQUIRE(planes == 1 || chroma64_dev, "mjpeg_encode_i420: null pointer (chroma table)");
    MjGeom g;
    SN_REQUIRE(N >= 1 && N <= 65535 && mj_geom(H, W, planes, 420, restart_mcus, &g),
               "mjpeg_encode_i420: bad batch, shape or restart interval (1..65535)");
    SN_REQUIRE(planes == 1 || ((H | W) & 1) == 0, "mjpeg_encode_i420: a 4:2:0 planar frame of %dx%d has an odd side, it needs even ones", W, H);
    const size_t fb = planes == 3 ? (size_t)H * W * 3 / 2 : (size_t)H * W;
    SN_REQUIRE(frame_stride_bytes >= fb, "mjpeg_encode_i420: frame_stride_bytes %zu < the frame's %zu bytes (%dx%d, %d plane%s)",
               frame_stride_bytes, fb, W, H, planes, planes == 1 ? "" : "s");
    const size_t need_out = stabnet_mjpeg_max_bytes(H, W, planes, 420, restart_mcus);
    SN_REQUIRE(header_bytes == mj_header_size(planes), "mjpeg_encode_i420: header_bytes %d, stabnet_mjpeg_header writes %d for C = %d", header_bytes,
               mj_header_size(planes), planes);
    SN_REQUIRE(out_stride >= need_out, "mjpeg_encode_i420: out_stride %zu < stabnet_mjpeg_max_bytes %zu", out_stride, need_out);
    const MjWs w = mj_ws(g);
    if (workspace_bytes < (size_t)N * w.frame) {
        stabnet_set_error("mjpeg_encode_i420: workspace %zu < %zu bytes", workspace_bytes, (size_t)N * w.frame);
        return STABNET_ERR_WORKSPACE;
    }
    SN_REQUIRE(((uintptr_t)workspace & 15) == 0, "mjpeg_encode_i420: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int rc = sn_check_device(src, "mjpeg_encode_i420: src", st);
    if (rc == 0) rc = sn_check_device(out, "mjpeg_encode_i420: out", st);
    if (rc == 0) rc = sn_check_device(workspace, "mjpeg_encode_i420: workspace", st);
    if (rc) return rc;
    Prof* prof = static_cast<Prof*>(profp);
    unsigned char* wsb = static_cast<unsigned char*>(workspace);
    short* coef = reinterpret_cast<short*>(wsb + w.coef);
    const size_t coef_stride = w.frame / sizeof(short);

    const bool rec = prof && prof->begin(st);
    {
        const dim3 grid(cdiv(cdiv(g.nmcu, g.mode == MJ_420 ? 1 : 8), 4), N);
        if (g.mode == MJ_420)
            mjpeg_transform_planar_kernel<MJ_420><<<grid, 256, 0, st>>>(src, frame_stride_bytes, H, W, g.mcux, g.nmcu, luma64_dev, chroma64_dev, coef, coef_stride);
        else
            mjpeg_transform_planar_kernel<MJ_GREY><<<grid, 256, 0, st>>>(src, frame_stride_bytes, H, W, g.mcux, g.nmcu, luma64_dev, luma64_dev, coef, coef_stride);
    }
    if (rec) prof->end(st, PK_KERNEL_MJPEG_TRANSFORM_PLANAR, 2.0 * 16.0 * (double)N * g.nblk * 64.0, (double)N * fb + (double)N * g.nblk * 128.0);
    SN_LAUNCH_CHECK("mjpeg_transform_planar_kernel");
    return mj_launch_tail(g, w, N, restart_mcus, wsb, header_dev, header_bytes, out, out_stride, out_bytes, st, prof);
}

}  // extern "C"
