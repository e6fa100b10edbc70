// Baseline JPEG (SOF0, 8-bit, Huffman; grey, 4:4:4, 4:2:0) decoder for Motion-JPEG input, gfx950, bit-exact with libjpeg-turbo's
// default decoder (JDCT_ISLOW, fancy upsampling): the compressed frame is uploaded and becomes the uint8 frame that stabnet_ingest_*
// reads, on the device.  The mirror image of mjpeg.hip.  N frames per call on the caller's stream; no host synchronisation,
// allocation or copy (capturable in a hipGraph with the ingest and the frame).  Per call: one memset node (the status words) and
//   mjpegd_entropy_kernel : one lane per restart interval (jpeg_entropy.h, the routine the host back end runs): Huffman tables of the
//                           stream's own DHT in LDS; int16 coefficients [mcu][block of the MCU][64], natural order, zero-filled
//                           (skipped when the caller uploads the coefficients of stabnet_mjpeg_entropy_host: streams without DRI)
//   mjpegd_idct_kernel    : eight lanes per block: dequantise, jidctint's 13-bit integer IDCT (columns, transpose through LDS, rows),
//                           + 128, clamp; uint8 planes at MCU-padded size
//   mjpegd_colour_kernel  : h2v2 fancy upsampling with neighbours clamped at the true chroma size, jdcolor's 16-bit fixed point,
//                           clamp; BGR or grey at the caller's row stride, four pixels per lane, dword stores where aligned
//   mjpegd_planes_kernel  : instead of the colour launch (stabnet_mjpeg_decode_i420): the MCU-padded planes cropped to the dense
//                           I420 frame Y [H,W] | U [H/2,W/2] | V [H/2,W/2] that stabnet_warp_rev_bundle2_i420 reads; no arithmetic
// Range: libjpeg looks the IDCT's result up in a table that wraps (& 1023) for values no real encoder produces; here it is a plain
// clamp to [0, 255].
#include "common.h"
#include "jpeg_tables.h"
#include "mjpeg_decode.h"
#include "prof.h"

namespace {

__constant__ const unsigned char d_zigzag[64] = JPEG_ZIGZAG_INIT;

// ---- entropy decoding ------------------------------------------------------------------------------------------------------------
// Workgroup b owns the intervals [256 b, 256 b + 256) of frame blockIdx.y, that is the MCUs [256 b R, 256 (b + 1) R): it zero-fills
// their coefficients together, then every lane decodes its interval.  Every offset of the blob is checked against the launch's
// geometry and the slot's size before it is used; a frame whose blob does not fit gets JD_ERR_BLOB and zero coefficients.
template <int MODE>
__global__ __launch_bounds__(256) void mjpegd_entropy_kernel(const unsigned char* __restrict__ in, size_t in_stride, int H, int W, int nmcu,
                                                             size_t blob_max, short* __restrict__ coef, size_t coef_frame_stride,
                                                             int* __restrict__ status) {
    constexpr int BPM = MODE == JD_MODE_420 ? 6 : (MODE == JD_MODE_444 ? 3 : 1);
    __shared__ __attribute__((aligned(16))) JdHuff s_huff[4];
    __shared__ unsigned char s_zz[64];
    __shared__ int s_sel[6];
    const int n = blockIdx.y;
    const unsigned char* slot = in + (size_t)n * in_stride;
    const JdBlobHead* hd = reinterpret_cast<const JdBlobHead*>(slot);
    const int R = hd->restart_mcus, nint = hd->nint, nbytes = hd->nbytes;
    bool ok = hd->magic == kJdMagic && hd->H == H && hd->W == W && hd->mode == MODE && hd->nmcu == nmcu && R >= 1 && R <= nmcu &&
              nint == (nmcu + R - 1) / R && nbytes >= 0 && blob_max + (size_t)nbytes <= in_stride &&
              kJdBlobStarts + ((size_t)nint + 1) * sizeof(int) <= blob_max;
#pragma unroll
    for (int c = 0; c < 3; ++c) ok = ok && (unsigned)hd->td[c] <= 1u && (unsigned)hd->ta[c] <= 1u;
    const int Rz = ok ? R : 1;
    {   // zero the coefficients of this workgroup's MCUs
        const long m0 = (long)blockIdx.x * 256 * Rz, m1 = min((long)nmcu, m0 + 256L * Rz);
        if (m0 < m1) {
            uint4* z = reinterpret_cast<uint4*>(coef + (size_t)n * coef_frame_stride + (size_t)m0 * BPM * 64);
            const long cnt = (m1 - m0) * BPM * 8;                         // 128 bytes per block
            for (long i = threadIdx.x; i < cnt; i += 256) z[i] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
    if (!ok) {
        if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(status + n, JD_ERR_BLOB);
        return;
    }
    {
        const unsigned* src = reinterpret_cast<const unsigned*>(slot + kJdBlobHuff);
        unsigned* dst = reinterpret_cast<unsigned*>(s_huff);
        for (int i = threadIdx.x; i < (int)(4 * sizeof(JdHuff) / 4); i += 256) dst[i] = src[i];
        if (threadIdx.x < 64) s_zz[threadIdx.x] = d_zigzag[threadIdx.x];
        if (threadIdx.x < 3) { s_sel[threadIdx.x] = hd->td[threadIdx.x]; s_sel[3 + threadIdx.x] = hd->ta[threadIdx.x]; }
    }
    __syncthreads();
    const int it = blockIdx.x * 256 + threadIdx.x;
    if (it >= nint) return;
    const int* starts = reinterpret_cast<const int*>(slot + kJdBlobStarts);
    const int a = starts[it], b = starts[it + 1] - 2;
    int st = JD_ERR_BLOB;
    if (a >= 0 && a <= b && b <= nbytes) {
        const int m0 = it * R, m1 = min(nmcu, m0 + R);
        st = jd_decode_interval(slot + blob_max, a, b, s_huff, s_sel, s_sel + 3, MODE, m1 - m0,
                                coef + (size_t)n * coef_frame_stride + (size_t)m0 * BPM * 64, s_zz);
    }
    if (st) atomicOr(status + n, st);
}

// ---- dequantisation + IDCT ---------------------------------------------------------------------------------------------------------
// jidctint.c (JDCT_ISLOW) in 32-bit integers: CONST_BITS 13, PASS1_BITS 2.  The zero-AC shortcuts of libjpeg give the same numbers
// as the full path, so there is none here.
__device__ __forceinline__ void jd_idct8(const int in[8], int out[8], int shift) {
    int z1 = (in[2] + in[6]) * 4433;
    const int tmp2 = z1 - in[6] * 15137, tmp3 = z1 + in[2] * 6270;
    const int tmp0 = (in[0] + in[4]) * 8192, tmp1 = (in[0] - in[4]) * 8192;            // << CONST_BITS
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    int a0 = in[7], a1 = in[5], a2 = in[3], a3 = in[1];
    z1 = a0 + a3;
    int z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const int z5 = (z3 + z4) * 9633;
    a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    const int rnd = 1 << (shift - 1);
    out[0] = (tmp10 + a3 + rnd) >> shift; out[7] = (tmp10 - a3 + rnd) >> shift;
    out[1] = (tmp11 + a2 + rnd) >> shift; out[6] = (tmp11 - a2 + rnd) >> shift;
    out[2] = (tmp12 + a1 + rnd) >> shift; out[5] = (tmp12 - a1 + rnd) >> shift;
    out[3] = (tmp13 + a0 + rnd) >> shift; out[4] = (tmp13 - a0 + rnd) >> shift;
}

// 32 blocks per workgroup, lane = (block, column) then (block, row).  A block sits in LDS with rows 9 ints apart and blocks 72 apart:
// the column pass writes word 72 b + 9 k + c and the row pass reads 72 b + 9 r + j, and over the 32 lanes that share an LDS cycle
// (4 blocks x 8) both hit 32 different banks.
constexpr int kIdctRow = 9, kIdctBlk = 72;

template <int MODE>
__global__ __launch_bounds__(256) void mjpegd_idct_kernel(const short* __restrict__ coef, size_t coef_frame_stride,
                                                          const unsigned char* __restrict__ in, size_t in_stride, int mcux, int nblk,
                                                          unsigned char* __restrict__ ws, size_t ws_frame, size_t yoff, size_t cboff,
                                                          size_t croff, int yw, int cw) {
    constexpr int BPM = MODE == JD_MODE_420 ? 6 : (MODE == JD_MODE_444 ? 3 : 1);
    __shared__ int s_blk[32 * kIdctBlk];
    __shared__ unsigned short s_q[3][64];
    const int n = blockIdx.y;
    {
        const JdBlobHead* hd = reinterpret_cast<const JdBlobHead*>(in + (size_t)n * in_stride);
        const unsigned short* q = reinterpret_cast<const unsigned short*>(in + (size_t)n * in_stride + kJdBlobQuant);
        if (threadIdx.x < 192) s_q[threadIdx.x >> 6][threadIdx.x & 63] = q[(hd->tq[threadIdx.x >> 6] & 3) * 64 + (threadIdx.x & 63)];
    }
    __syncthreads();
    const int lb = threadIdx.x >> 3, c = threadIdx.x & 7;
    const int blk = blockIdx.x * 32 + lb;
    const bool live = blk < nblk;
    const int m = blk / BPM, j = blk - m * BPM;
    const int comp = MODE == JD_MODE_GREY ? 0 : (MODE == JD_MODE_444 ? j : (j < 4 ? 0 : j - 3));
    int* sb = s_blk + lb * kIdctBlk;
    if (live) {
        const short* cf = coef + (size_t)n * coef_frame_stride + (size_t)blk * 64;
        int v[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (int)cf[k * 8 + c] * (int)s_q[comp][k * 8 + c];
        jd_idct8(v, o, 11);                                   // CONST_BITS - PASS1_BITS
#pragma unroll
        for (int k = 0; k < 8; ++k) sb[k * kIdctRow + c] = o[k];
    }
    __syncthreads();
    if (live) {
        const int r = c;
        int v[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = sb[r * kIdctRow + k];
        jd_idct8(v, o, 18);                                   // CONST_BITS + PASS1_BITS + 3
        unsigned w[2] = {0u, 0u};
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k >> 2] |= (unsigned)min(max(o[k] + 128, 0), 255) << (8 * (k & 3));
        const int my = m / mcux, mx = m - my * mcux;
        unsigned char* frame = ws + (size_t)n * ws_frame;
        size_t at;
        if (MODE == JD_MODE_420 && j < 4) at = yoff + (size_t)(my * 16 + (j >> 1) * 8 + r) * yw + mx * 16 + (j & 1) * 8;
        else if (comp == 0) at = yoff + (size_t)(my * 8 + r) * yw + mx * 8;
        else at = (comp == 1 ? cboff : croff) + (size_t)(my * 8 + r) * cw + mx * 8;
        *reinterpret_cast<uint2*>(frame + at) = make_uint2(w[0], w[1]);           // plane bases are 16-byte, widths 8-byte multiples
    }
}

// ---- upsampling + colour -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int jd_clamp8(int v) { return min(max(v, 0), 255); }

// One lane = four pixels of a row.  4:2:0: jdsample.c h2v2_fancy_upsample -- the chroma row r and its neighbour (r - 1 for even
// output rows, r + 1 for odd ones, clamped to the true chroma height) give s[c] = 3 C[r][c] + C[nb][c]; output 2c is
// (3 s[c] + s[c - 1] + 8) >> 4 and 2c + 1 is (3 s[c] + s[c + 1] + 7) >> 4, with c - 1, c + 1 clamped to the true chroma width.
template <int MODE>
__global__ __launch_bounds__(256) void mjpegd_colour_kernel(const unsigned char* __restrict__ ws, size_t ws_frame, size_t yoff, size_t cboff,
                                                            size_t croff, int yw, int cw, int H, int W, unsigned char* __restrict__ out,
                                                            size_t row_stride, size_t frame_stride) {
    constexpr int C = MODE == JD_MODE_GREY ? 1 : 3;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y, n = blockIdx.z;
    if (x0 >= W) return;
    const unsigned char* frame = ws + (size_t)n * ws_frame;
    const unsigned yy = *reinterpret_cast<const unsigned*>(frame + yoff + (size_t)y * yw + x0);       // yw is a multiple of 8
    int cb[4], cr[4];
    if (MODE == JD_MODE_444) {
        const unsigned b4 = *reinterpret_cast<const unsigned*>(frame + cboff + (size_t)y * cw + x0);
        const unsigned r4 = *reinterpret_cast<const unsigned*>(frame + croff + (size_t)y * cw + x0);
#pragma unroll
        for (int i = 0; i < 4; ++i) { cb[i] = (int)((b4 >> (8 * i)) & 0xffu); cr[i] = (int)((r4 >> (8 * i)) & 0xffu); }
    } else if (MODE == JD_MODE_420) {
        const int tch = (H + 1) >> 1, tcw = (W + 1) >> 1;                  // true chroma size
        const int r = y >> 1, nb = min(max((y & 1) ? r + 1 : r - 1, 0), tch - 1);
        const int c0 = x0 >> 1;
        int cc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) cc[i] = min(max(c0 - 1 + i, 0), tcw - 1);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const unsigned char* pl = frame + (p ? croff : cboff);
            int s[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) s[i] = 3 * (int)pl[(size_t)r * cw + cc[i]] + (int)pl[(size_t)nb * cw + cc[i]];
            // columns c0 (s[1]) and c0 + 1 (s[2]); past the last chroma column s[2] repeats s[1]'s clamp and feeds only pixels >= W
            int* o = p ? cr : cb;
            o[0] = (3 * s[1] + s[0] + 8) >> 4;
            o[1] = (3 * s[1] + s[2] + 7) >> 4;
            o[2] = (3 * s[2] + s[1] + 8) >> 4;
            o[3] = (3 * s[2] + s[3] + 7) >> 4;
        }
    }
    unsigned char px[4 * C];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int Y = (int)((yy >> (8 * i)) & 0xffu);
        if (MODE == JD_MODE_GREY) {
            px[i] = (unsigned char)Y;
        } else {
            const int b = cb[i] - 128, r = cr[i] - 128;
            px[i * C + 0] = (unsigned char)jd_clamp8(Y + ((116130 * b + 32768) >> 16));
            px[i * C + 1] = (unsigned char)jd_clamp8(Y + ((-22554 * b - 46802 * r + 32768) >> 16));
            px[i * C + 2] = (unsigned char)jd_clamp8(Y + ((91881 * r + 32768) >> 16));
        }
    }
    unsigned char* dst = out + (size_t)n * frame_stride + (size_t)y * row_stride + (size_t)x0 * C;
    if (x0 + 4 <= W && ((uintptr_t)dst & 3) == 0) {
        unsigned* d4 = reinterpret_cast<unsigned*>(dst);
#pragma unroll
        for (int k = 0; k < C; ++k)
            d4[k] = (unsigned)px[4 * k] | ((unsigned)px[4 * k + 1] << 8) | ((unsigned)px[4 * k + 2] << 16) | ((unsigned)px[4 * k + 3] << 24);
    } else {
        const int np = min(4, W - x0) * C;
#pragma unroll
        for (int k = 0; k < 4 * C; ++k)
            if (k < np) dst[k] = px[k];
    }
}

// The status words of the I420 entries are zeroed by a launch, not by a memset node: in a captured graph, the memset node of the BGR
// entries has been seen to leave a wrong value in the word on the graph's first replay (the frame itself was right), and a status the
// caller cannot trust is worth one tiny launch.
// (A template, so that it is emitted at its first use, behind the existing kernels: tools/isa_hash.py shows those unchanged that way.)
template <typename T>
__global__ __launch_bounds__(256) void mjpegd_clear_status_kernel(T* __restrict__ status, int N) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n < N) status[n] = T(0);
}

// ---- planes as they are --------------------------------------------------------------------------------------------------------------
// grid (cdiv(cdiv(W, 4), 256), H [+ 2 * (H / 2)], N): one workgroup per row segment of ONE plane, as remap_i420_kernel lays its grid
// out -- rows 0 .. H - 1 are the Y plane's, then the Cb plane's H / 2, then the Cr plane's.  One lane = four pixels of the row: one
// dword of the padded plane (its rows are 8-byte multiples on a 16-byte base, so the dword is aligned and inside the row), stored as a
// dword where the destination is aligned and the four pixels exist, as bytes otherwise.  Nothing outside the frame's own H * W * 3 / 2
// (grey: H * W) bytes is written.
template <int MODE>
__global__ __launch_bounds__(256) void mjpegd_planes_kernel(const unsigned char* __restrict__ ws, size_t ws_frame, size_t yoff, size_t cboff,
                                                            size_t croff, int yw, int cw, int H, int W, unsigned char* __restrict__ out,
                                                            size_t frame_stride) {
    const int n = blockIdx.z;
    int y = blockIdx.y, pw = W, sw = yw;
    size_t soff = yoff, doff = 0;
    if (MODE == JD_MODE_420 && y >= H) {                       // H, W even (the entry checks): chroma is H / 2 x W / 2
        const int CH = H >> 1;
        y -= H; pw = W >> 1; sw = cw;
        soff = cboff; doff = (size_t)H * W;
        if (y >= CH) { y -= CH; soff = croff; doff += (size_t)CH * pw; }
    }
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x0 >= pw) return;
    const unsigned v = *reinterpret_cast<const unsigned*>(ws + (size_t)n * ws_frame + soff + (size_t)y * sw + x0);
    unsigned char* dst = out + (size_t)n * frame_stride + doff + (size_t)y * pw + x0;
    if (x0 + 4 <= pw && ((uintptr_t)dst & 3) == 0) {
        *reinterpret_cast<unsigned*>(dst) = v;
    } else {
        const int np = min(4, pw - x0);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < np) dst[k] = (unsigned char)(v >> (8 * k));
    }
}

}  // namespace

extern "C" {

/* See include/stabnet_hip.h. */
size_t stabnet_mjpeg_decode_workspace_bytes(int N, int H, int W, int C, int subsampling) {
    JdGeom g;
    if (N < 1 || !jd_geom(H, W, C, subsampling, &g)) {
        stabnet_set_error("mjpeg_decode_workspace_bytes: bad batch, shape, channels or subsampling");
        return 0;
    }
    return (size_t)N * g.frame;
}

int stabnet_mjpeg_decode_layout(int H, int W, int C, int subsampling, size_t* layout10) {
    JdGeom g;
    SN_REQUIRE(layout10, "mjpeg_decode_layout: null pointer");
    SN_REQUIRE(jd_geom(H, W, C, subsampling, &g), "mjpeg_decode_layout: bad shape, channels or subsampling");
    const size_t v[10] = {g.frame, g.coef, g.nblk, g.yoff, g.cboff, g.croff, (size_t)g.yh, (size_t)g.yw, (size_t)g.ch, (size_t)g.cw};
    for (int i = 0; i < 10; ++i) layout10[i] = v[i];
    return STABNET_OK;
}

int stabnet_mjpeg_decode(const unsigned char* in, size_t in_stride, int N, int H, int W, int C, int subsampling, int coef_uploaded,
                         unsigned char* out, size_t row_stride, size_t frame_stride, int* status, void* workspace, size_t workspace_bytes,
                         int stages, void* stream) {
    SN_REQUIRE(in && status && workspace, "mjpeg_decode: null pointer");
    JdGeom g;
    SN_REQUIRE(N >= 1 && N <= 65535 && jd_geom(H, W, C, subsampling, &g), "mjpeg_decode: bad batch, shape, channels (1 | 3) or subsampling (420 | 444)");
    SN_REQUIRE(stages >= 1 && stages <= 3, "mjpeg_decode: stages must be 1 (entropy), 2 (+ IDCT) or 3 (+ colour: the frame)");
    SN_REQUIRE(stages < 3 || out, "mjpeg_decode: null pointer (out)");
    SN_REQUIRE(stages < 3 || (row_stride >= (size_t)W * C && (N == 1 || frame_stride >= (size_t)(H - 1) * row_stride + (size_t)W * C)),
               "mjpeg_decode: row_stride %zu / frame_stride %zu too small for %dx%dx%d", row_stride, frame_stride, H, W, C);
    const size_t coef_bytes = g.nblk * 64 * sizeof(short);
    SN_REQUIRE((in_stride & 15) == 0 && ((uintptr_t)in & 15) == 0, "mjpeg_decode: in and in_stride must be 16-byte aligned");
    SN_REQUIRE(in_stride >= g.blob_max + (coef_uploaded ? coef_bytes : 0), "mjpeg_decode: in_stride %zu < %zu", in_stride,
               g.blob_max + (coef_uploaded ? coef_bytes : 0));
    if (workspace_bytes < (size_t)N * g.frame) {
        stabnet_set_error("mjpeg_decode: workspace %zu < %zu bytes", workspace_bytes, (size_t)N * g.frame);
        return STABNET_ERR_WORKSPACE;
    }
    SN_REQUIRE(((uintptr_t)workspace & 15) == 0, "mjpeg_decode: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int rc = sn_check_device(in, "mjpeg_decode: in", st);
    if (rc == 0 && out) rc = sn_check_device(out, "mjpeg_decode: out", st);
    if (rc == 0) rc = sn_check_device(workspace, "mjpeg_decode: workspace", st);
    if (rc == 0) rc = sn_check_device(status, "mjpeg_decode: status", st);
    if (rc) return rc;
    unsigned char* wsb = static_cast<unsigned char*>(workspace);
    if (hipMemsetAsync(status, 0, (size_t)N * sizeof(int), st) != hipSuccess) {
        stabnet_set_error("mjpeg_decode: hipMemsetAsync failed");
        return STABNET_ERR_LAUNCH;
    }
    const short* coef = reinterpret_cast<const short*>(wsb + g.coef);
    size_t coef_stride = g.frame / sizeof(short);
    if (coef_uploaded) {                     // the slot holds blob | coefficients: the IDCT reads them where they were uploaded
        coef = reinterpret_cast<const short*>(in + g.blob_max);
        coef_stride = in_stride / sizeof(short);
    } else {
        const dim3 grid(cdiv(g.nmcu, 256), N);
        short* cw = reinterpret_cast<short*>(wsb + g.coef);
        if (g.mode == JD_MODE_420)
            mjpegd_entropy_kernel<JD_MODE_420><<<grid, 256, 0, st>>>(in, in_stride, H, W, g.nmcu, g.blob_max, cw, coef_stride, status);
        else if (g.mode == JD_MODE_444)
            mjpegd_entropy_kernel<JD_MODE_444><<<grid, 256, 0, st>>>(in, in_stride, H, W, g.nmcu, g.blob_max, cw, coef_stride, status);
        else
            mjpegd_entropy_kernel<JD_MODE_GREY><<<grid, 256, 0, st>>>(in, in_stride, H, W, g.nmcu, g.blob_max, cw, coef_stride, status);
        SN_LAUNCH_CHECK("mjpegd_entropy_kernel");
    }
    return mjpegd_launch_planes(g, H, W, in, in_stride, N, coef, coef_stride, wsb, out, row_stride, frame_stride, stages, stream);
}

/* See include/stabnet_hip.h. */
int stabnet_mjpeg_decode_i420(const unsigned char* in, size_t in_stride, int N, int H, int W, int C, int subsampling, int coef_uploaded,
                              unsigned char* out, size_t frame_stride_bytes, int* status, void* workspace, size_t workspace_bytes, void* stream,
                              void* prof) {
    SN_REQUIRE(in && out && status && workspace, "mjpeg_decode_i420: null pointer");
    JdGeom g;
    int rc = mjpegd_i420_geom("mjpeg_decode_i420", N, H, W, C, subsampling, frame_stride_bytes, &g);
    if (rc) return rc;
    const size_t coef_bytes = g.nblk * 64 * sizeof(short);
    SN_REQUIRE((in_stride & 15) == 0 && ((uintptr_t)in & 15) == 0, "mjpeg_decode_i420: in and in_stride must be 16-byte aligned");
    SN_REQUIRE(in_stride >= g.blob_max + (coef_uploaded ? coef_bytes : 0), "mjpeg_decode_i420: in_stride %zu < %zu", in_stride,
               g.blob_max + (coef_uploaded ? coef_bytes : 0));
    if (workspace_bytes < (size_t)N * g.frame) {
        stabnet_set_error("mjpeg_decode_i420: workspace %zu < %zu bytes", workspace_bytes, (size_t)N * g.frame);
        return STABNET_ERR_WORKSPACE;
    }
    SN_REQUIRE(((uintptr_t)workspace & 15) == 0, "mjpeg_decode_i420: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    rc = sn_check_device(in, "mjpeg_decode_i420: in", st);
    if (rc == 0) rc = sn_check_device(out, "mjpeg_decode_i420: out", st);
    if (rc == 0) rc = sn_check_device(workspace, "mjpeg_decode_i420: workspace", st);
    if (rc == 0) rc = sn_check_device(status, "mjpeg_decode_i420: status", st);
    if (rc) return rc;
    unsigned char* wsb = static_cast<unsigned char*>(workspace);
    rc = mjpegd_clear_status(status, N, stream);
    if (rc) return rc;
    const short* coef = reinterpret_cast<const short*>(wsb + g.coef);
    size_t coef_stride = g.frame / sizeof(short);
    if (coef_uploaded) {                     // the slot holds blob | coefficients: the IDCT reads them where they were uploaded
        coef = reinterpret_cast<const short*>(in + g.blob_max);
        coef_stride = in_stride / sizeof(short);
    } else {
        const dim3 grid(cdiv(g.nmcu, 256), N);
        short* cw = reinterpret_cast<short*>(wsb + g.coef);
        if (g.mode == JD_MODE_420)
            mjpegd_entropy_kernel<JD_MODE_420><<<grid, 256, 0, st>>>(in, in_stride, H, W, g.nmcu, g.blob_max, cw, coef_stride, status);
        else
            mjpegd_entropy_kernel<JD_MODE_GREY><<<grid, 256, 0, st>>>(in, in_stride, H, W, g.nmcu, g.blob_max, cw, coef_stride, status);
        SN_LAUNCH_CHECK("mjpegd_entropy_kernel");
    }
    return mjpegd_launch_i420(g, H, W, in, in_stride, N, coef, coef_stride, wsb, out, frame_stride_bytes, stream, prof);
}

}  // extern "C"

// The launches behind the entropy decoding (stages 2 and 3), for stabnet_mjpeg_decode and stabnet_mjpeg_decode_sync alike.  Defined
// behind the entries: kernels are emitted in the order of their first use, and tools/isa_hash.py shows them unchanged that way.
int mjpegd_launch_planes(const JdGeom& g, int H, int W, const unsigned char* in, size_t in_stride, int N, const short* coef, size_t coef_stride,
                         unsigned char* wsb, unsigned char* out, size_t row_stride, size_t frame_stride, int stages, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (stages < 2) return STABNET_OK;
    {
        const dim3 grid(cdiv((long)g.nblk, 32), N);
        if (g.mode == JD_MODE_420)
            mjpegd_idct_kernel<JD_MODE_420><<<grid, 256, 0, st>>>(coef, coef_stride, in, in_stride, g.mcux, (int)g.nblk, wsb, g.frame, g.yoff, g.cboff, g.croff, g.yw, g.cw);
        else if (g.mode == JD_MODE_444)
            mjpegd_idct_kernel<JD_MODE_444><<<grid, 256, 0, st>>>(coef, coef_stride, in, in_stride, g.mcux, (int)g.nblk, wsb, g.frame, g.yoff, g.cboff, g.croff, g.yw, g.cw);
        else
            mjpegd_idct_kernel<JD_MODE_GREY><<<grid, 256, 0, st>>>(coef, coef_stride, in, in_stride, g.mcux, (int)g.nblk, wsb, g.frame, g.yoff, g.cboff, g.croff, g.yw, g.cw);
        SN_LAUNCH_CHECK("mjpegd_idct_kernel");
    }
    if (stages < 3) return STABNET_OK;
    {
        const dim3 grid(cdiv(cdiv(W, 4), 256), H, N);
        if (g.mode == JD_MODE_420)
            mjpegd_colour_kernel<JD_MODE_420><<<grid, 256, 0, st>>>(wsb, g.frame, g.yoff, g.cboff, g.croff, g.yw, g.cw, H, W, out, row_stride, frame_stride);
        else if (g.mode == JD_MODE_444)
            mjpegd_colour_kernel<JD_MODE_444><<<grid, 256, 0, st>>>(wsb, g.frame, g.yoff, g.cboff, g.croff, g.yw, g.cw, H, W, out, row_stride, frame_stride);
        else
            mjpegd_colour_kernel<JD_MODE_GREY><<<grid, 256, 0, st>>>(wsb, g.frame, g.yoff, g.cboff, g.croff, g.yw, g.cw, H, W, out, row_stride, frame_stride);
        SN_LAUNCH_CHECK("mjpegd_colour_kernel");
    }
    return STABNET_OK;
}

// What stabnet_mjpeg_decode_i420 and stabnet_mjpeg_decode_sync_i420 accept, judged before any launch: grey of any size, 4:2:0 with even
// sides, frames that do not overlap.
int mjpegd_i420_geom(const char* who, int N, int H, int W, int C, int subsampling, size_t frame_stride, JdGeom* g) {
    SN_REQUIRE(N >= 1 && N <= 65535 && jd_geom(H, W, C, subsampling, g), "%s: bad batch, shape, channels (1 | 3) or subsampling (420 | 444)", who);
    SN_REQUIRE(g->mode != JD_MODE_444, "%s: 4:4:4 streams have no I420 frame; stabnet_mjpeg_decode reads them (BGR)", who);
    SN_REQUIRE(g->mode != JD_MODE_420 || ((H | W) & 1) == 0,
               "%s: a 4:2:0 stream of %dx%d has an odd side, a dense I420 frame needs even ones; stabnet_mjpeg_decode reads it (BGR)", who, W, H);
    const size_t fb = g->mode == JD_MODE_420 ? (size_t)H * W * 3 / 2 : (size_t)H * W;
    SN_REQUIRE(frame_stride >= fb, "%s: frame_stride_bytes %zu < the frame's %zu bytes (%dx%d, %d plane%s)", who, frame_stride, fb, W, H, C,
               C == 1 ? "" : "s");
    return STABNET_OK;
}

// The IDCT launch and the crop to the dense I420 frame, behind any entropy back end.
int mjpegd_launch_i420(const JdGeom& g, int H, int W, const unsigned char* in, size_t in_stride, int N, const short* coef, size_t coef_stride,
                       unsigned char* wsb, unsigned char* out, size_t frame_stride, void* stream, void* profp) {
    hipStream_t st = (hipStream_t)stream;
    const int rc = mjpegd_launch_planes(g, H, W, in, in_stride, N, coef, coef_stride, wsb, nullptr, 0, 0, 2, stream);
    if (rc) return rc;
    Prof* prof = static_cast<Prof*>(profp);
    const bool rec = prof && prof->begin(st);
    const dim3 grid(cdiv(cdiv(W, 4), 256), g.mode == JD_MODE_420 ? H + 2 * (H / 2) : H, N);
    if (g.mode == JD_MODE_420)
        mjpegd_planes_kernel<JD_MODE_420><<<grid, 256, 0, st>>>(wsb, g.frame, g.yoff, g.cboff, g.croff, g.yw, g.cw, H, W, out, frame_stride);
    else
        mjpegd_planes_kernel<JD_MODE_GREY><<<grid, 256, 0, st>>>(wsb, g.frame, g.yoff, g.cboff, g.croff, g.yw, g.cw, H, W, out, frame_stride);
    // bytes: the dwords read of the padded planes (the frame's size rounded up per row) + the frame written
    if (rec) prof->end(st, PK_KERNEL_MJPEGD_PLANES, 0.0, 2.0 * (double)N * (g.mode == JD_MODE_420 ? 1.5 : 1.0) * H * W);
    SN_LAUNCH_CHECK("mjpegd_planes_kernel");
    return STABNET_OK;
}

int mjpegd_clear_status(int* status, int N, void* stream) {
    mjpegd_clear_status_kernel<int><<<cdiv(N, 256), 256, 0, (hipStream_t)stream>>>(status, N);
    SN_LAUNCH_CHECK("mjpegd_clear_status_kernel");
    return STABNET_OK;
}
