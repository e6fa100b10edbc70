// Colour-frame remap with smoothed maps (deploy_bundle.py:136-146 warpRevBundle2), gfx950.
// The reference does this on the host with OpenCV after every sess.run; here the maps never leave the device:
//   map_shrink_kernel : cv2.resize(map, (W/rate, H/rate)) INTER_LINEAR (half-pixel centres, float32, h-pass then v-pass)
//   remap_*_kernel    : cv2.resize back up fused with (m+1)/2*size and cv2.remap(..., INTER_LINEAR) on the uint8 frame: OpenCV's
//                       FIXED-POINT bilinear path, BORDER_CONSTANT 0 -- integer arithmetic, bit-exact against the oracle
// Float32 op order of the two resizes as oracle/stabnet_oracle.py: cv_resize_linear_f32 (-ffp-contract=off).  HBM-bound:
// per frame 8*H*W (maps in) + 3*H*W (frame, gathered) + 3*H*W (out) bytes.
#include <cmath>
#include <cstdlib>
#include "common.h"
#include "prof.h"

struct Taps1D { int i0, i1; float w0, w1; };

// e: the destination position in pixel-edge units (pixel d covers [d, d + 1), its centre is d + 0.5)
__device__ __forceinline__ Taps1D cv_taps_at(double e, int n_src, double scale) {
    float f = (float)(e * scale - 0.5);
    int s = (int)floorf(f);
    f = f - (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= n_src - 1) { f = 0.f; s = n_src - 1; }
    Taps1D t;
    t.i0 = s; t.i1 = min(s + 1, n_src - 1); t.w0 = 1.0f - f; t.w1 = f;
    return t;
}

__device__ __forceinline__ Taps1D cv_taps(int d, int n_src, double scale) { return cv_taps_at((double)d + 0.5, n_src, scale); }

__device__ __forceinline__ float cv_resize_at(const float* __restrict__ src, int sw, const Taps1D& tx, const Taps1D& ty) {
    const float r0 = src[(size_t)ty.i0 * sw + tx.i0] * tx.w0 + src[(size_t)ty.i0 * sw + tx.i1] * tx.w1;
    const float r1 = src[(size_t)ty.i1 * sw + tx.i0] * tx.w0 + src[(size_t)ty.i1 * sw + tx.i1] * tx.w1;
    return r0 * ty.w0 + r1 * ty.w1;
}

// small[n][0|1][h][w] <- x_map, y_map shrunk.  One thread per low-resolution pixel.
__global__ __launch_bounds__(256) void map_shrink_kernel(const float* __restrict__ x_map, const float* __restrict__ y_map, int H,
                                                         int W, int h, int w, float* __restrict__ small_maps) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y;
    if (q >= h * w) return;
    const int dy = q / w, dx = q - dy * w;
    const Taps1D tx = cv_taps(dx, W, (double)W / w), ty = cv_taps(dy, H, (double)H / h);
    small_maps[((size_t)n * 2 + 0) * h * w + q] = cv_resize_at(x_map + (size_t)n * H * W, W, tx, ty);
    small_maps[((size_t)n * 2 + 1) * h * w + q] = cv_resize_at(y_map + (size_t)n * H * W, W, tx, ty);
}

// ---- the remap itself, stated once for all eight kernels below ----
// small = cv2.resize(map, (w, h)) (map_shrink_kernel); big = cv2.resize(small, (SW, SH)); network-pixel coordinate
// u = (big + 1) / 2 * size; then cv2.remap(..., INTER_LINEAR) on the uint8 frame.  At SOURCE resolution (the frame as read: [SH, SW, C],
// any size, strided rows) the source-pixel coordinate under cv2's half-pixel convention is p = u * s + c with s = SW / W and
// c = 0.5 * SW / W - 0.5 (the reference's normalised coordinate counts pixel INDICES: without c an identity mesh would shift the picture
// by 0.5 * (SW / W - 1) source pixels); both constants rounded once from double by the host, multiply then add, not fused.  With
// SH, SW == H, W: s = 1, c = 0, and the network-size kernels (AFFINE = false) skip the step: p is u's own bits.
struct SrcRemapArgs {
    int SH, SW, C, H, W, h, w;
    float fW, fH, sx, cx, sy, cy;            // (float)W, (float)H; float32(SW / W), float32(0.5 * SW / W - 0.5), likewise y
    double xscale, yscale;                   // (double)w / SW, (double)h / SH: cv_taps of the resize back up
    size_t row_stride, frame_stride;         // bytes
};

struct SrcCoord { float px, py; int qx, qy; };   // qx, qy: the coordinate in 1/32 px, rounded half to even

// The coordinate cv2.remap receives, and OpenCV's quantisation of it to 1/32 px (cvRound: half to even).  (A float beyond the int range
// is out of frame either way: clamped before the conversion.)
template <bool AFFINE = true>
__device__ __forceinline__ SrcCoord remap_src_coord(const float* __restrict__ mx, const float* __restrict__ my,
        const SrcRemapArgs& a, const Taps1D& tx, const Taps1D& ty) {
    const float xs = cv_resize_at(mx, a.w, tx, ty), ys = cv_resize_at(my, a.w, tx, ty);
    const float ux = (xs + 1.0f) / 2.0f * a.fW;                     // deploy_bundle.py:142-143
    const float uy = (ys + 1.0f) / 2.0f * a.fH;
    SrcCoord c;
    c.px = AFFINE ? ux * a.sx + a.cx : ux;
    c.py = AFFINE ? uy * a.sy + a.cy : uy;
    const float qx = fminf(fmaxf(c.px * 32.0f, -2.0e9f), 2.0e9f), qy = fminf(fmaxf(c.py * 32.0f, -2.0e9f), 2.0e9f);
    c.qx = (qx == qx) ? (int)rintf(qx) : -2000000000;
    c.qy = (qy == qy) ? (int)rintf(qy) : -2000000000;
    return c;
}

// coverage: the rounded coordinate lies outside the frame (a NaN map entry too: -2e9)
__device__ __forceinline__ bool remap_src_black(const SrcCoord& c, int SH, int SW) {
    return c.qx < 0 || c.qx > 32 * (SW - 1) || c.qy < 0 || c.qy > 32 * (SH - 1);
}

// OpenCV's 8-bit bilinear remap (imgwarp.cpp: RemapInvoker + remapBilinear<FixedPtCast<int, uchar, 15>, RemapVec_8u, short>;
// oracle cv_remap_linear_u8 / cv_bilinear_tab_i) of a coordinate in 1/32 px: integer part saturated to int16, 15-bit integer weights
// wy[k1] * wx[k2] * 32768 -- all exact multiples of 32 except the table's entry (0, 0), whose weight 1.0 saturates to 32767 and whose
// repair loop puts the missing 1 on tap [1][1] -- BORDER_CONSTANT 0 for the taps outside the frame, integer accumulate, (sum + 16384) >> 15.
struct RemapTaps { int ix, iy, w00, w01, w10, w11; };          // top-left pixel, the weights of taps [row][column]
__device__ __forceinline__ RemapTaps remap_taps(const SrcCoord& c) {
    RemapTaps t; t.ix = min(max(c.qx >> 5, -32768), 32767); t.iy = min(max(c.qy >> 5, -32768), 32767);
    const int fx = c.qx & 31, fy = c.qy & 31;
    t.w00 = (32 - fy) * (32 - fx) * 32; t.w01 = (32 - fy) * fx * 32; t.w10 = fy * (32 - fx) * 32; t.w11 = fy * fx * 32;
    if ((fx | fy) == 0) { t.w00 = 32767; t.w11 = 1; }
    return t;
}

__device__ __forceinline__ unsigned remap_blend(int v00, int v01, int v10, int v11, int w00, int w01, int w10, int w11) {
    const int acc = (v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11 + (1 << 14)) >> 15;
    return (unsigned)min(max(acc, 0), 255);
}

// ---- the bicubic taps (--interp cubic): cv2.remap(..., INTER_CUBIC), OpenCV's fixed-point path (imgwarp.cpp: initInterTab2D(INTER_CUBIC,
// fixpt = true) + remapBicubic<FixedPtCast<int, uchar, 15>, short, 32768>; tests/remap_cubic_model.py).  The coordinate and its
// quantisation are the bilinear path's; the 16 taps sit at rows iy - 1 .. iy + 2, columns ix - 1 .. ix + 2, and their weights are entry
// (fy, fx) of BicubicTab_i: saturate_cast<short>(rint(float32(cy[k1] * cx[k2]) * 32768)) of the two 1-D rows interpolateCubic(f / 32)
// (A = -0.75, float32, left to right, not contracted), then the table's repair: an entry whose taps do not sum to 32768 (657 of the
// 1024) has the difference taken from the smallest (sum too large) or largest (too small) of taps [2..3][2..3].  Signed weights: the
// blend clamps at both ends.
// The kernels read the 32 KiB int16 table from global memory, two 16-byte loads per pixel (measured 3-13 % faster per launch than forming
// the weights in registers: profiles/r20_remap_cubic_weights_ab.txt).  The table is a CONSTANT of the code object, evaluated by the compiler
// from the functions below (IEEE float32, nothing contracted): no upload, no state per device, nothing to do before a graph is captured.
// The host builder (stabnet_remap_cubic_table) runs the same functions at run time; the tests hold both to the NumPy model.
constexpr __host__ __device__ void cubic_coeffs(int i, float* c) {
    const float A = -0.75f, x = (float)i * (1.f / 32);
    c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

// rint of |v| < 2^23, half to even (v - (float)i is exact there); constexpr, unlike rintf
constexpr __host__ __device__ int cubic_rint(float v) {
    const int i = (int)v;
    const float r = v - (float)i;
    if (r > 0.5f || (r == 0.5f && (i & 1))) return i + 1;
    if (r < -0.5f || (r == -0.5f && (i & 1))) return i - 1;
    return i;
}

// w[k1 * 4 + k2]: the weight of the tap at row iy - 1 + k1, column ix - 1 + k2
constexpr __host__ __device__ void cubic_weights_calc(int fx, int fy, int* w) {
    float cx[4] = {}, cy[4] = {};
    cubic_coeffs(fx, cx); cubic_coeffs(fy, cy);
    int sum = 0;
    for (int k1 = 0; k1 < 4; ++k1)
        for (int k2 = 0; k2 < 4; ++k2) {
            const float v = cy[k1] * cx[k2];
            int iv = cubic_rint(v * 32768.0f);
            iv = iv < -32768 ? -32768 : (iv > 32767 ? 32767 : iv);       // saturate_cast<short>: entry (0, 0)'s 1.0 becomes 32767
            w[k1 * 4 + k2] = iv; sum += iv;
        }
    // the repair loop of initInterTab2D with ksize = 4: k1, k2 in {2, 3} in row order, the minimum with strict <, otherwise the maximum
    // with strict >, both starting at tap [2][2]; diff == 0 leaves the entry alone
    const int diff = sum - 32768;
    int mk = 10, Mk = 10;
    for (int k = 0; k < 4; ++k) {
        const int t = 10 + (k & 1) + 4 * (k >> 1);
        if (w[t] < w[mk]) mk = t;
        else if (w[t] > w[Mk]) Mk = t;
    }
    w[diff < 0 ? Mk : mk] -= diff;
}

struct alignas(16) CubicTab { short w[1024 * 16]; };         // entry fy * 32 + fx, tap k1 * 4 + k2
constexpr CubicTab cubic_make_tab() {
    CubicTab t = {};
    for (int e = 0; e < 1024; ++e) {
        int w[16] = {};
        cubic_weights_calc(e & 31, e >> 5, w);
        for (int k = 0; k < 16; ++k) t.w[e * 16 + k] = (short)w[k];
    }
    return t;
}
__device__ const CubicTab g_cubic_tab = cubic_make_tab();

__device__ __forceinline__ void cubic_weights(int fx, int fy, int* w) {
    const int4* p = reinterpret_cast<const int4*>(g_cubic_tab.w + ((fy * 32 + fx) << 4));
    const int4 a = p[0], b = p[1];
    const int v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) { w[2 * k] = (v[k] << 16) >> 16; w[2 * k + 1] = v[k] >> 16; }
}

__device__ __forceinline__ unsigned remap_cubic_round(int acc) { return (unsigned)min(max((acc + (1 << 14)) >> 15, 0), 255); }

// One channel of one pixel by byte loads: im the frame (or plane), pixels C bytes apart; a tap outside reads `border`.
__device__ __forceinline__ unsigned remap_cubic_px(const unsigned char* __restrict__ im, size_t row_stride, int C, int ch, int SH, int SW, int ix,
        int iy, const int* w, int border) {
    int acc = 0;
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) {
        const int yy = iy - 1 + k1;
        const bool oky = yy >= 0 && yy < SH;
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2) {
            const int xx = ix - 1 + k2;
            const int v = (oky && xx >= 0 && xx < SW) ? (int)im[(size_t)yy * row_stride + (size_t)xx * C + ch] : border;
            acc += v * w[k1 * 4 + k2];
        }
    }
    return remap_cubic_round(acc);
}

// The four BGR taps of row yy from pixel x0 on: 12 contiguous bytes in three dwords, border 0.  All four inside the row: the four
// aligned dwords that cover them where they lie inside [lo, hi) (the frame's own bytes), funnel-shifted; bytes otherwise, and tap by
// tap where the row's end cuts the taps.  Nothing outside [lo, hi) is read.
struct Bytes12 { unsigned d[3]; };
__device__ __forceinline__ Bytes12 remap_cubic_row12(const unsigned char* __restrict__ im, size_t row_stride, int yy, int x0, int SH, int SW,
        const unsigned char* lo, const unsigned char* hi) {
    Bytes12 b; b.d[0] = 0u; b.d[1] = 0u; b.d[2] = 0u;
    if (yy < 0 || yy >= SH || x0 + 3 < 0 || x0 >= SW) return b;
    const unsigned char* row = im + (size_t)yy * row_stride;
    if (x0 >= 0 && x0 + 3 < SW) {
        const unsigned char* p = row + (size_t)x0 * 3;
        const uintptr_t al = (uintptr_t)p & ~(uintptr_t)3;
        const int sh = 8 * (int)((uintptr_t)p & 3);
        if (al >= (uintptr_t)lo && al + 16 <= (uintptr_t)hi) {
            const unsigned* q = reinterpret_cast<const unsigned*>(al);
            const unsigned q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
            b.d[0] = (unsigned)(((((unsigned long long)q1) << 32) | q0) >> sh);
            b.d[1] = (unsigned)(((((unsigned long long)q2) << 32) | q1) >> sh);
            b.d[2] = (unsigned)(((((unsigned long long)q3) << 32) | q2) >> sh);
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) b.d[k >> 2] |= ((unsigned)p[k]) << (8 * (k & 3));
        }
        return b;
    }
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2) {
        const int xx = x0 + k2;
        if (xx < 0 || xx >= SW) continue;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) b.d[(k2 * 3 + ch) >> 2] |= ((unsigned)row[(size_t)xx * 3 + ch]) << (8 * ((k2 * 3 + ch) & 3));
    }
    return b;
}

// The same for a dense plane (C == 1, rows SW bytes apart): four bytes in one dword, a tap outside reads `border`.
__device__ __forceinline__ unsigned remap_cubic_row4(const unsigned char* __restrict__ im, int yy, int x0, int SH, int SW, unsigned border) {
    if (yy < 0 || yy >= SH || x0 + 3 < 0 || x0 >= SW) return border * 0x01010101u;
    const unsigned char* row = im + (size_t)yy * SW;
    const unsigned char* hi = im + (size_t)SH * SW;
    unsigned r = 0u;
    if (x0 >= 0 && x0 + 3 < SW) {
        const unsigned char* p = row + x0;
        const uintptr_t al = (uintptr_t)p & ~(uintptr_t)3;
        const int sh = 8 * (int)((uintptr_t)p & 3);
        if (al >= (uintptr_t)im && al + 8 <= (uintptr_t)hi) {
            const unsigned* q = reinterpret_cast<const unsigned*>(al);
            const unsigned q0 = q[0], q1 = q[1];
            return (unsigned)(((((unsigned long long)q1) << 32) | q0) >> sh);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) r |= ((unsigned)p[k]) << (8 * k);
        return r;
    }
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2) {
        const int xx = x0 + k2;
        r |= ((xx >= 0 && xx < SW) ? (unsigned)row[xx] : border) << (8 * k2);
    }
    return r;
}

// One pixel: output pixel `pix` of stream n, its taps into the small maps given.  Any C, width, stride and alignment; byte loads and stores.
// CUBIC: the 16 taps above in place of the four bilinear ones; everything else is shared.
template <bool AFFINE, bool CUBIC = false>
__device__ __forceinline__ void remap_pixel(const unsigned char* __restrict__ src, const SrcRemapArgs& a,
        const float* __restrict__ small_maps, int n, const Taps1D& tx, const Taps1D& ty, size_t pix, unsigned char* __restrict__ out,
        int* __restrict__ black_count, float* __restrict__ px_out, float* __restrict__ py_out) {
    const int C = a.C;
    const size_t hw = (size_t)a.h * a.w;
    const SrcCoord c = remap_src_coord<AFFINE>(small_maps + ((size_t)n * 2 + 0) * hw, small_maps + ((size_t)n * 2 + 1) * hw, a, tx, ty);
    if (px_out != nullptr) { px_out[pix] = c.px; py_out[pix] = c.py; }
    const RemapTaps t = remap_taps(c);
    if constexpr (CUBIC) {
        const unsigned char* im = src + (size_t)n * a.frame_stride;
        int w[16];
        cubic_weights(c.qx & 31, c.qy & 31, w);
        for (int ch = 0; ch < C; ++ch) out[pix * C + ch] = (unsigned char)remap_cubic_px(im, a.row_stride, C, ch, a.SH, a.SW, t.ix, t.iy, w, 0);
    } else {
        const bool x0 = t.ix >= 0 && t.ix < a.SW, x1 = t.ix + 1 >= 0 && t.ix + 1 < a.SW, y0 = t.iy >= 0 && t.iy < a.SH, y1 = t.iy + 1 >= 0 && t.iy + 1 < a.SH;
        const unsigned char* im = src + (size_t)n * a.frame_stride;
        for (int ch = 0; ch < C; ++ch) {
            const int v00 = (x0 && y0) ? (int)im[(size_t)t.iy * a.row_stride + (size_t)t.ix * C + ch] : 0;
            const int v01 = (x1 && y0) ? (int)im[(size_t)t.iy * a.row_stride + (size_t)(t.ix + 1) * C + ch] : 0;
            const int v10 = (x0 && y1) ? (int)im[(size_t)(t.iy + 1) * a.row_stride + (size_t)t.ix * C + ch] : 0;
            const int v11 = (x1 && y1) ? (int)im[(size_t)(t.iy + 1) * a.row_stride + (size_t)(t.ix + 1) * C + ch] : 0;
            out[pix * C + ch] = (unsigned char)remap_blend(v00, v01, v10, v11, t.w00, t.w01, t.w10, t.w11);
        }
    }
    if (black_count != nullptr && remap_src_black(c, a.SH, a.SW)) black_count[pix] += 1;
}

// bytes p .. p+5 in the low 48 bits (lo <= p, p + 3 <= hi; [lo, hi) = the frame's own bytes): the three aligned dwords that cover
// them where all three lie inside [lo, hi) (p may sit at byte 3 of its dword), funnel-shifted; bytes otherwise (a frame that starts or
// ends inside a dword: any base pointer and row stride are accepted, and nothing outside the frame is read)
__device__ __forceinline__ unsigned long long remap_src_load6(const unsigned char* __restrict__ p, const unsigned char* lo, const unsigned char* hi) {
    const uintptr_t al = (uintptr_t)p & ~(uintptr_t)3;
    const int sh = 8 * (int)((uintptr_t)p & 3);
    if (al >= (uintptr_t)lo && al + 12 <= (uintptr_t)hi) {
        const unsigned* q = reinterpret_cast<const unsigned*>(al);
        const unsigned d0 = q[0], d1 = q[1], d2 = q[2];
        const unsigned l = (unsigned)(((((unsigned long long)d1) << 32) | d0) >> sh), h = (unsigned)(((((unsigned long long)d2) << 32) | d1) >> sh);
        return (((unsigned long long)h) << 32) | l;
    }
    unsigned long long r = 0ull;
    for (int k = 0; k < 6; ++k)
        if (p + k < hi) r |= ((unsigned long long)p[k]) << (8 * k);
    return r;
}

// Four consecutive output pixels from `pix` on (C == 3, the row's width % 4 == 0, out 4-byte aligned, px_out / py_out 16-byte: the colour
// frames of the path); taps_x(e) gives the horizontal taps of pixel e.  The byte traffic of remap_pixel -- 12 one-byte gathers and 3
// one-byte stores per pixel -- becomes 4-byte traffic: the two taps of a row are 6 CONTIGUOUS bytes (BGR BGR), fetched through
// remap_src_load6 (the source may have any width, stride and alignment); the 12 output bytes of the four pixels leave as three 4-byte
// stores of one thread.  Same integer arithmetic, same results.  CUBIC: the four taps of a row are 12 contiguous bytes
// (remap_cubic_row12), four rows per pixel; the stores are the same three.
template <bool AFFINE, bool CUBIC = false, class TapsX>
__device__ __forceinline__ void remap_pixel4(const unsigned char* __restrict__ src, const SrcRemapArgs& a,
        const float* __restrict__ small_maps, int n, TapsX taps_x, const Taps1D& ty, size_t pix, unsigned char* __restrict__ out,
        int* __restrict__ black_count, float* __restrict__ px_out, float* __restrict__ py_out) {
    const int SH = a.SH, SW = a.SW;
    const size_t hw = (size_t)a.h * a.w;
    const float* mx = small_maps + ((size_t)n * 2 + 0) * hw;
    const float* my = small_maps + ((size_t)n * 2 + 1) * hw;
    const unsigned char* im = src + (size_t)n * a.frame_stride;
    const unsigned char* end = im + (size_t)(SH - 1) * a.row_stride + (size_t)SW * 3;
    unsigned ob[3] = {0u, 0u, 0u};                           // the 12 output bytes
    float pxs[4], pys[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const SrcCoord c = remap_src_coord<AFFINE>(mx, my, a, taps_x(e), ty);
        pxs[e] = c.px; pys[e] = c.py;
        // remap_taps' statements in place: through the function the compiler orders the last pixel's instructions differently, and
        // remap_win4_dev_kernel then measured half a timer tick over the parent's range (profiles/remap_refactor_ab.txt)
        const int ix = min(max(c.qx >> 5, -32768), 32767), iy = min(max(c.qy >> 5, -32768), 32767);
        const int fx = c.qx & 31, fy = c.qy & 31;
        if constexpr (CUBIC) {
            int w[16], acc[3] = {0, 0, 0};
            cubic_weights(fx, fy, w);
#pragma unroll
            for (int k1 = 0; k1 < 4; ++k1) {
                const Bytes12 b = remap_cubic_row12(im, a.row_stride, iy - 1 + k1, ix - 1, SH, SW, im, end);
#pragma unroll
                for (int k = 0; k < 12; ++k) acc[k % 3] += (int)((b.d[k >> 2] >> (8 * (k & 3))) & 0xffu) * w[k1 * 4 + k / 3];
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                unsigned o = remap_cubic_round(acc[ch]);
                asm volatile("" : "+v"(o));                  // the byte finished in its own register before packing (see remap_plane_pixels)
                const int byte = e * 3 + ch;
                ob[byte >> 2] |= o << (8 * (byte & 3));
            }
            if (black_count != nullptr && remap_src_black(c, SH, SW)) black_count[pix + e] += 1;
            continue;
        }
        int w00 = (32 - fy) * (32 - fx) * 32, w01 = (32 - fy) * fx * 32, w10 = fy * (32 - fx) * 32, w11 = fy * fx * 32;
        if ((fx | fy) == 0) { w00 = 32767; w11 = 1; }
        const bool vx0 = ix >= 0 && ix < SW, vx1 = ix + 1 >= 0 && ix + 1 < SW, vy0 = iy >= 0 && iy < SH, vy1 = iy + 1 >= 0 && iy + 1 < SH;
        // rows iy and iy + 1: 6 bytes from pixel max(ix, 0) on (ix == -1: the first three bytes are tap 1)
        unsigned long long r0 = 0ull, r1 = 0ull;
        const int cx = max(ix, 0);
        if ((vx0 || vx1) && vy0) r0 = remap_src_load6(im + (size_t)iy * a.row_stride + (size_t)cx * 3, im, end);
        if ((vx0 || vx1) && vy1) r1 = remap_src_load6(im + (size_t)(iy + 1) * a.row_stride + (size_t)cx * 3, im, end);
        if (ix < 0) { r0 <<= 24; r1 <<= 24; }                // tap 0 out of frame on the left: what was loaded is tap 1
        const unsigned long long m0 = vx0 ? 0xffffffull : 0ull, m1 = vx1 ? 0xffffff000000ull : 0ull;
        r0 &= (vy0 ? (m0 | m1) : 0ull);
        r1 &= (vy1 ? (m0 | m1) : 0ull);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const unsigned o = remap_blend((int)((r0 >> (8 * ch)) & 0xff), (int)((r0 >> (24 + 8 * ch)) & 0xff), (int)((r1 >> (8 * ch)) & 0xff),
                                           (int)((r1 >> (24 + 8 * ch)) & 0xff), w00, w01, w10, w11);
            const int byte = e * 3 + ch;
            ob[byte >> 2] |= o << (8 * (byte & 3));
        }
        if (black_count != nullptr && remap_src_black(c, SH, SW)) black_count[pix + e] += 1;
    }
    unsigned* op = reinterpret_cast<unsigned*>(out + pix * 3);
    op[0] = ob[0]; op[1] = ob[1]; op[2] = ob[2];
    if (px_out != nullptr) {
        *reinterpret_cast<float4*>(px_out + pix) = make_float4(pxs[0], pxs[1], pxs[2], pxs[3]);
        *reinterpret_cast<float4*>(py_out + pix) = make_float4(pys[0], pys[1], pys[2], pys[3]);
    }
}

// ---- at the network's size: img [N, H, W, C] dense, a built for SH, SW == H, W (no coverage count).  Flat grid (cdiv(H * W, 256), N) ----
__global__ __launch_bounds__(256) void remap_color_kernel(const unsigned char* __restrict__ img, SrcRemapArgs a, const float* __restrict__ small_maps,
        unsigned char* __restrict__ out, float* __restrict__ px_out, float* __restrict__ py_out) {
    const int q = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    if (q >= a.SH * a.SW) return;
    const int y = q / a.SW, x = q - y * a.SW;
    remap_pixel<false>(img, a, small_maps, n, cv_taps(x, a.w, a.xscale), cv_taps(y, a.h, a.yscale), (size_t)n * a.SH * a.SW + q, out, nullptr,
                       px_out, py_out);
}

// grid (cdiv(H * W / 4, 256), N): C == 3, W % 4 == 0, img and out 4-byte aligned (px_out / py_out 16-byte)
__global__ __launch_bounds__(256) void remap_color4_kernel(const unsigned char* __restrict__ img, SrcRemapArgs a,
        const float* __restrict__ small_maps, unsigned char* __restrict__ out, float* __restrict__ px_out, float* __restrict__ py_out) {
    const int q4 = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y, W4 = a.SW >> 2;           // q4: group of four pixels
    if (q4 >= a.SH * W4) return;
    const int y = q4 / W4, x0 = (q4 - y * W4) * 4;
    remap_pixel4<false>(img, a, small_maps, n, [&](int e) { return cv_taps(x0 + e, a.w, a.xscale); }, cv_taps(y, a.h, a.yscale),
                        (size_t)n * a.SH * a.SW + (size_t)y * a.SW + x0, out, nullptr, px_out, py_out);
}

// ---- at SOURCE resolution, and through a WINDOW of the stabilised frame (crop and zoom in the one gather) ----
// Output pixel (i, j) of OH x OW is the stabilised frame (SH x SW) sampled at the position, in pixel-edge units,
//   ex = x0 + (j + 0.5) * (ww / OW),  ey = y0 + (i + 0.5) * (wh / OH)        (double; quotient, multiply, add)
// and that position takes the place of d + 0.5 in the taps of the resize back up (cv_taps_at); every other step is the same.  With the
// whole-frame window (0, 0, SH, SW) at OH, OW == SH, SW, ex = j + 0.5 exactly: every bit is stabnet_warp_rev_bundle2_src's (whose
// kernels take d + 0.5 itself: WINDOW = false); with an integer window at zoom 1, ex = x0 + j + 0.5 exactly: the slice of that result.
// And _src with SH, SW == H, W is stabnet_warp_rev_bundle2, bit for bit.  Coverage is counted at the OUTPUT pixel.
// The window of one launch as the body reads it: from the kernel arguments (remap_win_kernel, remap_win4_kernel) or from the stream's
// four doubles in device memory (remap_win_dev_kernel, remap_win4_dev_kernel).
struct WinSteps { double x0, y0, xstep, ystep; };      // xstep = ww / OW, ystep = wh / OH
struct WinRemapArgs { SrcRemapArgs a; int OH, OW; WinSteps ws; };

// grid (cdiv(OW / PX, blockDim.x), OH, N), one workgroup per row segment: the vertical taps and the two small-map rows are wave-uniform.
// PX consecutive output pixels per thread: 1, or 4 under remap_pixel4's preconditions on OW and out.
template <int PX, bool WINDOW, bool CUBIC = false>
__device__ __forceinline__ void remap_row_body(const unsigned char* __restrict__ src, const SrcRemapArgs& a, int OH, int OW, const WinSteps& ws,
        const float* __restrict__ small_maps, unsigned char* __restrict__ out, int* __restrict__ black_count, float* __restrict__ px_out,
        float* __restrict__ py_out) {
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * PX, y = blockIdx.y, n = blockIdx.z;
    if (x >= OW) return;
    auto taps_x = [&](int e) { return WINDOW ? cv_taps_at(ws.x0 + ((double)(x + e) + 0.5) * ws.xstep, a.w, a.xscale) : cv_taps(x + e, a.w, a.xscale); };
    const Taps1D ty = WINDOW ? cv_taps_at(ws.y0 + ((double)y + 0.5) * ws.ystep, a.h, a.yscale) : cv_taps(y, a.h, a.yscale);
    const size_t pix = ((size_t)n * OH + y) * OW + x;
    if constexpr (PX == 4) remap_pixel4<true, CUBIC>(src, a, small_maps, n, taps_x, ty, pix, out, black_count, px_out, py_out);
    else remap_pixel<true, CUBIC>(src, a, small_maps, n, taps_x(0), ty, pix, out, black_count, px_out, py_out);
}

__global__ __launch_bounds__(256) void remap_src_kernel(const unsigned char* __restrict__ src, SrcRemapArgs a, const float* __restrict__ small_maps,
        unsigned char* __restrict__ out, int* __restrict__ black_count, float* __restrict__ px_out, float* __restrict__ py_out) {
    remap_row_body<1, false>(src, a, a.SH, a.SW, WinSteps{}, small_maps, out, black_count, px_out, py_out);
}

__global__ __launch_bounds__(256) void remap_src4_kernel(const unsigned char* __restrict__ src, SrcRemapArgs a, const float* __restrict__ small_maps,
        unsigned char* __restrict__ out, int* __restrict__ black_count, float* __restrict__ px_out, float* __restrict__ py_out) {
    remap_row_body<4, false>(src, a, a.SH, a.SW, WinSteps{}, small_maps, out, black_count, px_out, py_out);
}

__global__ __launch_bounds__(256) void remap_win_kernel(const unsigned char* __restrict__ src, WinRemapArgs wa, const float* __restrict__ small_maps,
        unsigned char* __restrict__ out, int* __restrict__ black_count, float* __restrict__ px_out, float* __restrict__ py_out) {
    remap_row_body<1, true>(src, wa.a, wa.OH, wa.OW, wa.ws, small_maps, out, black_count, px_out, py_out);
}

__global__ __launch_bounds__(256) void remap_win4_kernel(const unsigned char* __restrict__ src, WinRemapArgs wa, const float* __restrict__ small_maps,
        unsigned char* __restrict__ out, int* __restrict__ black_count, float* __restrict__ px_out, float* __restrict__ py_out) {
    remap_row_body<4, true>(src, wa.a, wa.OH, wa.OW, wa.ws, small_maps, out, black_count, px_out, py_out);
}

// ---- the window in DEVICE memory: window[n] = {y0, x0, wh, ww}, four doubles per stream, written by an earlier launch on the stream
// (fill_window_kernel below) -- a captured graph freezes kernel arguments, not what a pointer among them points at.  The loads are
// workgroup-uniform (n = blockIdx.z); the two quotients are IEEE double divisions, the bits of the host's in stabnet_warp_rev_bundle2_win.
// A window the host entry would have refused (a non-finite entry, wh <= 0 or ww <= 0, one that leaves the frame by more than 1e-6 px)
// cannot be refused here: the launch reads the whole frame (0, 0, SH, SW) instead, and no tap is ever derived from a NaN.
__device__ __forceinline__ WinSteps remap_win_load(const double* __restrict__ window, int n, int SH, int SW, int OH, int OW) {
    double y0 = window[4 * (size_t)n + 0], x0 = window[4 * (size_t)n + 1], wh = window[4 * (size_t)n + 2], ww = window[4 * (size_t)n + 3];
    const bool finite = fabs(y0) <= 1.0e300 && fabs(x0) <= 1.0e300 && fabs(wh) <= 1.0e300 && fabs(ww) <= 1.0e300;   // false for NaN and Inf
    const bool ok = finite && wh > 0.0 && ww > 0.0 && y0 >= -1e-6 && x0 >= -1e-6 && y0 + wh <= (double)SH + 1e-6 && x0 + ww <= (double)SW + 1e-6;
    if (!ok) { y0 = 0.0; x0 = 0.0; wh = (double)SH; ww = (double)SW; }
    WinSteps ws;
    ws.x0 = x0; ws.y0 = y0; ws.xstep = ww / (double)OW; ws.ystep = wh / (double)OH;
    return ws;
}

// grids and preconditions as remap_win_kernel / remap_win4_kernel; wa.ws is not read
__global__ __launch_bounds__(256) void remap_win_dev_kernel(const unsigned char* __restrict__ src, WinRemapArgs wa, const double* __restrict__ window,
        const float* __restrict__ small_maps, unsigned char* __restrict__ out, int* __restrict__ black_count, float* __restrict__ px_out,
        float* __restrict__ py_out) {
    const WinSteps ws = remap_win_load(window, blockIdx.z, wa.a.SH, wa.a.SW, wa.OH, wa.OW);
    remap_row_body<1, true>(src, wa.a, wa.OH, wa.OW, ws, small_maps, out, black_count, px_out, py_out);
}

__global__ __launch_bounds__(256) void remap_win4_dev_kernel(const unsigned char* __restrict__ src, WinRemapArgs wa,
        const double* __restrict__ window, const float* __restrict__ small_maps, unsigned char* __restrict__ out, int* __restrict__ black_count,
        float* __restrict__ px_out, float* __restrict__ py_out) {
    const WinSteps ws = remap_win_load(window, blockIdx.z, wa.a.SH, wa.a.SW, wa.OH, wa.OW);
    remap_row_body<4, true>(src, wa.a, wa.OH, wa.OW, ws, small_maps, out, black_count, px_out, py_out);
}

// ---- the same six row-segment kernels with the bicubic taps (stabnet_warp_rev_bundle2_cubic).  KIND 0: the whole frame at its own size
// (remap_src_kernel's body), 1: the window in wa.ws, 2: the window loaded from device memory; `window` is read by KIND 2 only.
template <int PX, int KIND>
__global__ __launch_bounds__(256) void remap_cubic_kernel(const unsigned char* __restrict__ src, WinRemapArgs wa, const double* __restrict__ window,
        const float* __restrict__ small_maps, unsigned char* __restrict__ out, int* __restrict__ black_count, float* __restrict__ px_out,
        float* __restrict__ py_out) {
    if constexpr (KIND == 2) {
        const WinSteps ws = remap_win_load(window, blockIdx.z, wa.a.SH, wa.a.SW, wa.OH, wa.OW);
        remap_row_body<PX, true, true>(src, wa.a, wa.OH, wa.OW, ws, small_maps, out, black_count, px_out, py_out);
    } else {
        remap_row_body<PX, KIND == 1, true>(src, wa.a, wa.OH, wa.OW, wa.ws, small_maps, out, black_count, px_out, py_out);
    }
}

// out[(fy * 32 + fx) * 16 + k]: the weights of every phase exactly as the kernels above form them.  One thread per phase.
__global__ __launch_bounds__(256) void remap_cubic_weights_kernel(short* __restrict__ out) {
    const int e = blockIdx.x * 256 + threadIdx.x;            // grid 4: 1024 phases
    int w[16];
    cubic_weights(e & 31, e >> 5, w);
#pragma unroll
    for (int k = 0; k < 16; ++k) out[e * 16 + k] = (short)w[k];
}

// ---- adaptive borderless output: the largest centred window of one frame that is provably free of uncovered pixels ----
// The remap reads the h x w small maps through bilinear taps with non-negative weights that sum to one (the border clamps put the
// weight on one node), so the coordinate at ANY output position is a convex combination of the four surrounding nodes' coordinates;
// "covered" is an axis-aligned box; so a position whose four nodes lie inside the box lies inside it.  Node (a, b) is BAD when its own
// coordinate (remap_src_coord with the taps i0 = i1 = node, w0 = 1, w1 = 0) leaves the box shrunk by margin_q 1/32 px (the float
// rounding of the blend moves qx by far less).  A bad node b reaches the positions with tap coordinate f in (b - 1, b + 1); a centred
// window of ratio r reads f in (w/2 (1 - r) - 0.5, w/2 (1 + r) - 0.5): it avoids the node in x iff r w <= |2b + 1 - w| - 2, in y iff
// r h <= |2a + 1 - h| - 2, and avoiding it in either axis is enough.  Over the common denominator h w, in int32:
//   key(a, b) = max((|2b + 1 - w| - 2) h, (|2a + 1 - h| - 2) w),   key = min over the bad nodes (h w when there is none)
// One workgroup per stream strides over the nodes; min / sum through wave shuffles, then LDS: no atomics, no init launch, one order.
// Thread 0 then moves the stream's window (plain double arithmetic, in this order):
//   r_safe = key >= h w ? 1 : key / (h w);   r = fmin(r_safe, state + up);  r = fmax(r, r_min);  r = fmin(r, 1);   state = r
//   wh = SH r;  ww = SW r;  y0 = (SH - wh) / 2;  x0 = (SW - ww) / 2          (warp.ratio_window's expression)
// zooming in at once (no uncovered pixel whenever r_safe >= r_min), back out by at most `up` per frame.
struct FillArgs {
    SrcRemapArgs a;                          // C and the strides are not read
    int margin_q;
    double r_min, up;
};

__global__ __launch_bounds__(1024) void fill_window_kernel(const float* __restrict__ small_maps, FillArgs fa, double* __restrict__ state,
                                                           double* __restrict__ window, int* __restrict__ stats) {
    __shared__ int s_key[16], s_bad[16];
    const SrcRemapArgs& a = fa.a;
    const int n = blockIdx.x, h = a.h, w = a.w, nodes = h * w;
    const float* mx = small_maps + ((size_t)n * 2 + 0) * nodes;
    const float* my = small_maps + ((size_t)n * 2 + 1) * nodes;
    const int lo = fa.margin_q, xhi = 32 * (a.SW - 1) - fa.margin_q, yhi = 32 * (a.SH - 1) - fa.margin_q;
    int key = nodes, bad = 0;
    for (int q = threadIdx.x; q < nodes; q += blockDim.x) {
        const int na = q / w, nb = q - na * w;
        Taps1D tx, ty;
        tx.i0 = nb; tx.i1 = nb; tx.w0 = 1.0f; tx.w1 = 0.0f;
        ty.i0 = na; ty.i1 = na; ty.w0 = 1.0f; ty.w1 = 0.0f;
        const SrcCoord c = remap_src_coord(mx, my, a, tx, ty);
        if (c.qx < lo || c.qx > xhi || c.qy < lo || c.qy > yhi) {
            key = min(key, max((abs(2 * nb + 1 - w) - 2) * h, (abs(2 * na + 1 - h) - 2) * w));
            ++bad;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        key = min(key, __shfl_xor(key, off));
        bad += __shfl_xor(bad, off);
    }
    const int wave = threadIdx.x >> 6, waves = blockDim.x >> 6;      // blockDim.x is a multiple of 64, at most 1024
    if ((threadIdx.x & 63) == 0) { s_key[wave] = key; s_bad[wave] = bad; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < waves; ++k) { key = min(key, s_key[k]); bad += s_bad[k]; }
    const double r_safe = key >= nodes ? 1.0 : (double)key / (double)nodes;          // may be <= 0
    double r = fmin(r_safe, state[n] + fa.up);
    r = fmax(r, fa.r_min);
    r = fmin(r, 1.0);
    state[n] = r;
    const double wh = (double)a.SH * r, ww = (double)a.SW * r;
    window[4 * (size_t)n + 0] = ((double)a.SH - wh) / 2.0;
    window[4 * (size_t)n + 1] = ((double)a.SW - ww) / 2.0;
    window[4 * (size_t)n + 2] = wh;
    window[4 * (size_t)n + 3] = ww;
    stats[2 * (size_t)n + 0] = key;
    stats[2 * (size_t)n + 1] = bad;
}

// cvt_train2img (deploy_bundle.py:75): ((x + 0.5) * 255).astype(uint8), clipped to [0, 255] first (the network's grey output is a
// bilinear blend of inputs in [-0.5, 0.5], so the clip only guards the cast).  4 pixels per thread, float4 in, one dword out.
__global__ __launch_bounds__(256) void cvt_train2img_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, long n) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    auto cv = [](float v) -> unsigned int { return (unsigned int)fminf(fmaxf((v + 0.5f) * 255.0f, 0.0f), 255.0f); };
    if (i + 4 <= n && (((uintptr_t)x | (uintptr_t)out) & 15) == 0) {
        const float4 v = *reinterpret_cast<const float4*>(x + i);
        *reinterpret_cast<unsigned int*>(out + i) = cv(v.x) | (cv(v.y) << 8) | (cv(v.z) << 16) | (cv(v.w) << 24);
    } else {
        for (long j = i; j < n && j < i + 4; ++j) out[j] = (unsigned char)cv(x[j]);
    }
}

// ---- a planar YUV 4:2:0 frame (I420: the Y plane [SH, SW], then U and V [SH/2, SW/2], all dense), every plane in ONE launch ----
// Each plane is what remap_win_kernel gives it as a C == 1 image of the plane's own size: the Y plane at (SH, SW) -> (OH, OW) through the
// window, a chroma plane at (SH/2, SW/2) -> (OH/2, OW/2) through the halved window with its own sx, cx, sy, cy (src_remap_args of the
// plane's size) -- with centred chroma siting that is the luma coordinate of the chroma sample, halved.  One difference: a tap outside
// the plane reads a BORDER VALUE instead of 0 (cv2.remap's borderValue): (Y, U, V) = (0, 0, 0) is saturated green, so chroma reads 128.
// Coverage is counted at the luma output pixel.  The window is always given (the whole frame: steps of exactly 1, _src's bits).
struct I420Geom { SrcRemapArgs a; int OH, OW; WinSteps ws; };        // one plane kind: a.C == 1, a.row_stride == a.SW
struct I420Args {
    I420Geom g[2];                           // luma, chroma
    size_t src_off[3], out_off[3];           // of planes Y, U, V inside a frame, bytes
    size_t src_frame, out_frame;             // bytes from one frame to the next
    int px4[3];                              // the plane takes the four-pixel path: its OW % 4 == 0 and its output rows are 4-byte aligned
    int border[3];
};

// PX consecutive output pixels of row y of one plane from x on; orow, black_row: the row's first output byte / count (or null)
template <int PX, bool CUBIC = false>
__device__ __forceinline__ void remap_plane_pixels(const unsigned char* __restrict__ im, const I420Geom& g, const float* __restrict__ mx,
        const float* __restrict__ my, int x, int y, int border, unsigned char* __restrict__ orow, int* __restrict__ black_row) {
    const SrcRemapArgs& a = g.a;
    const Taps1D ty = cv_taps_at(g.ws.y0 + ((double)y + 0.5) * g.ws.ystep, a.h, a.yscale);
    unsigned ob = 0u;
#pragma unroll
    for (int e = 0; e < PX; ++e) {
        const Taps1D tx = cv_taps_at(g.ws.x0 + ((double)(x + e) + 0.5) * g.ws.xstep, a.w, a.xscale);
        const SrcCoord c = remap_src_coord<true>(mx, my, a, tx, ty);
        const RemapTaps t = remap_taps(c);
        unsigned o;
        if constexpr (CUBIC) {
            int w[16];
            cubic_weights(c.qx & 31, c.qy & 31, w);
            if constexpr (PX == 4) {                          // the four taps of a row are one dword
                int acc = 0;
#pragma unroll
                for (int k1 = 0; k1 < 4; ++k1) {
                    const unsigned r = remap_cubic_row4(im, t.iy - 1 + k1, t.ix - 1, a.SH, a.SW, (unsigned)border);
#pragma unroll
                    for (int k2 = 0; k2 < 4; ++k2) acc += (int)((r >> (8 * k2)) & 0xffu) * w[k1 * 4 + k2];
                }
                o = remap_cubic_round(acc);
            } else {
                o = remap_cubic_px(im, (size_t)a.SW, 1, 0, a.SH, a.SW, t.ix, t.iy, w, border);
            }
        } else {
            const bool x0 = t.ix >= 0 && t.ix < a.SW, x1 = t.ix + 1 >= 0 && t.ix + 1 < a.SW, y0 = t.iy >= 0 && t.iy < a.SH, y1 = t.iy + 1 >= 0 && t.iy + 1 < a.SH;
            const int v00 = (x0 && y0) ? (int)im[(size_t)t.iy * a.SW + t.ix] : border;
            const int v01 = (x1 && y0) ? (int)im[(size_t)t.iy * a.SW + t.ix + 1] : border;
            const int v10 = (x0 && y1) ? (int)im[(size_t)(t.iy + 1) * a.SW + t.ix] : border;
            const int v11 = (x1 && y1) ? (int)im[(size_t)(t.iy + 1) * a.SW + t.ix + 1] : border;
            o = remap_blend(v00, v01, v10, v11, t.w00, t.w01, t.w10, t.w11);
        }
        if constexpr (PX == 4) {
            // The byte is finished in a register of its own before it is packed (an empty statement the compiler cannot see through).
            // Left to itself, hipcc folds the shift and clamp of pixels 0 and 1 into one v_ashr_pk_u8_i32 on the first accumulator's own
            // register and ORs pixels 2 and 3 into the result as if its bits 31:16 were zero; on the MI355X they still held bits 31:16
            // of that accumulator, so pixel 2 came out as value | (acc0 >> 16) & 0xff (seen against the one-pixel path and the model).
            asm volatile("" : "+v"(o));
            ob |= o << (8 * e);
        } else {
            orow[x] = (unsigned char)o;
        }
        if (black_row != nullptr && remap_src_black(c, a.SH, a.SW)) black_row[x + e] += 1;
    }
    if constexpr (PX == 4) *reinterpret_cast<unsigned*>(orow + x) = ob;
}

// grid (cdiv(items, blockDim.x), OH [+ 2 * (OH / 2)], N): one workgroup per row segment of ONE plane -- rows 0 .. OH - 1 are the Y plane's,
// then the U plane's OH / 2, then the V plane's -- so the plane, its path and its vertical taps are workgroup-uniform.  items: the most
// any plane needs (OW / 4 or OW threads for a Y row, half of that for a chroma row on the same path).
// CUBIC: the bicubic taps on every plane (stabnet_warp_rev_bundle2_i420_cubic).  (One templated kernel, not a shared body behind two kernels:
// handing the by-value I420Args on to a function changed the bilinear kernel's code.)
template <bool CUBIC>
__global__ __launch_bounds__(256) void remap_i420_kernel(const unsigned char* __restrict__ src, I420Args ia, const float* __restrict__ small_maps,
        unsigned char* __restrict__ out, int* __restrict__ black_count) {
    const int n = blockIdx.z, OH = ia.g[0].OH, CH = ia.g[1].OH;
    int y = blockIdx.y, plane = 0;
    if (y >= OH) { y -= OH; plane = 1; if (y >= CH) { y -= CH; plane = 2; } }
    const I420Geom& g = ia.g[plane != 0];
    const int t = blockIdx.x * blockDim.x + threadIdx.x, px4 = ia.px4[plane];
    const int x = px4 ? t * 4 : t;
    if (x >= g.OW) return;
    const size_t hw = (size_t)g.a.h * g.a.w;
    const float* mx = small_maps + ((size_t)n * 2 + 0) * hw;
    const float* my = small_maps + ((size_t)n * 2 + 1) * hw;
    const unsigned char* im = src + (size_t)n * ia.src_frame + ia.src_off[plane];
    unsigned char* orow = out + (size_t)n * ia.out_frame + ia.out_off[plane] + (size_t)y * g.OW;
    int* black_row = (plane == 0 && black_count != nullptr) ? black_count + ((size_t)n * OH + y) * g.OW : nullptr;
    if (px4) remap_plane_pixels<4, CUBIC>(im, g, mx, my, x, y, ia.border[plane], orow, black_row);
    else remap_plane_pixels<1, CUBIC>(im, g, mx, my, x, y, ia.border[plane], orow, black_row);
}

// STABNET_REMAP_VEC4=0: the one-pixel-per-thread kernels everywhere (debug switch; read once)
static int remap_vec4_enabled() {
    static const int v4 = []() { const char* v = getenv("STABNET_REMAP_VEC4"); return v ? atoi(v) : 1; }();
    return v4;
}

// the change of coordinates of the source-resolution remaps: every constant computed in double, rounded once
static void src_remap_args(SrcRemapArgs& a, int SH, int SW, int C, int H, int W, int h, int w, size_t row_stride_bytes) {
    a.SH = SH; a.SW = SW; a.C = C; a.H = H; a.W = W; a.h = h; a.w = w;
    a.fW = (float)W; a.fH = (float)H;
    a.sx = (float)((double)SW / (double)W); a.cx = (float)(0.5 * (double)SW / (double)W - 0.5);
    a.sy = (float)((double)SH / (double)H); a.cy = (float)(0.5 * (double)SH / (double)H - 0.5);
    a.xscale = (double)w / SW; a.yscale = (double)h / SH;
    a.row_stride = row_stride_bytes; a.frame_stride = (size_t)SH * row_stride_bytes;
}

// the four-pixel kernels take BGR rows of a multiple of 4 pixels whose 12 output bytes (and 4 coordinates) land aligned
static bool remap_vec4(int C, int width, const void* out, const float* px_out, const float* py_out) {
    const bool aligned = ((size_t)out & 3) == 0 && (px_out == nullptr || (((size_t)px_out | (size_t)py_out) & 15) == 0);
    return remap_vec4_enabled() && C == 3 && width % 4 == 0 && aligned;
}

static int remap_shrink(const float* x_map, const float* y_map, int N, int H, int W, int h, int w, float* workspace, hipStream_t st, Prof* prof) {
    const bool rec = prof && prof->begin(st);
    map_shrink_kernel<<<dim3(cdiv(h * w, 256), N), 256, 0, st>>>(x_map, y_map, H, W, h, w, workspace);
    if (rec) prof->end(st, PK_KERNEL_MAP_SHRINK, 0.0, (double)N * 8.0 * ((double)H * W + (double)h * w));
    SN_LAUNCH_CHECK("map_shrink_kernel");
    return STABNET_OK;
}

// stabnet_warp_rev_bundle2_src, _win and _win_dev are one entry: the same checks in the same order, the shrink, then the kind's pair of
// kernels over row segments of the output.  _src is the whole frame at its own size (window not read, OH, OW == SH, SW).
enum RemapKind { REMAP_SRC, REMAP_WIN, REMAP_WIN_DEV };

// stabnet_warp_rev_bundle2_cubic is the same entry again (cubic: its three window kinds are the three kinds), launching the bicubic kernels.
static int remap_src_entry(RemapKind kind, bool cubic, const unsigned char* src, int N, int SH, int SW, int C, size_t row_stride_bytes,
                           const float* x_map, const float* y_map, int H, int W, int rate, const double* window, int OH, int OW, unsigned char* out,
                           int* black_count, float* workspace, float* px_out, float* py_out, void* stream, void* profp) {
#define REMAP_NAMES(n) {n, n ": src", n ": out", n ": workspace", n ": window"}
    static const struct { const char *who, *src, *out, *workspace, *window; } all_names[4] = {
        REMAP_NAMES("warp_rev_bundle2_src"), REMAP_NAMES("warp_rev_bundle2_win"), REMAP_NAMES("warp_rev_bundle2_win_dev"),
        REMAP_NAMES("warp_rev_bundle2_cubic")};
#undef REMAP_NAMES
    const auto& nm = all_names[cubic ? 3 : kind];
    const char* who = nm.who;
    SN_REQUIRE(src && x_map && y_map && out && workspace, "%s: null pointer", who);
    SN_REQUIRE(kind == REMAP_SRC || window != nullptr, "%s: null window", who);
    SN_REQUIRE(C == 1 || C == 3, "%s: C must be 1 (grey) or 3 (BGR), got %d", who, C);
    SN_REQUIRE(N >= 1 && N <= 65535, "%s: batch %d outside 1..65535", who, N);
    SN_REQUIRE(SH >= 1 && SH <= 32767 && SW >= 1 && SW <= 32767, "%s: source %dx%d outside 1..32767 (the remap's 16-bit pixel index)", who, SH, SW);
    SN_REQUIRE(OH >= 1 && OH <= 32767 && OW >= 1 && OW <= 32767, "%s: output %dx%d outside 1..32767", who, OH, OW);
    SN_REQUIRE(kind != REMAP_SRC || (OH == SH && OW == SW), "%s: window_kind 0 is the whole frame at its own size, got output %dx%d of source %dx%d",
               who, OH, OW, SH, SW);
    SN_REQUIRE(H >= 1 && W >= 1 && rate >= 1 && H / rate >= 1 && W / rate >= 1, "%s: maps %dx%d leave nothing at rate %d", who, H, W, rate);
    SN_REQUIRE(row_stride_bytes >= (size_t)SW * C, "%s: row stride %zu < %d * %d bytes", who, row_stride_bytes, SW, C);
    SN_REQUIRE((px_out == nullptr) == (py_out == nullptr), "%s: px_out and py_out go together", who);
    double y0 = 0.0, x0 = 0.0, wh = (double)SH, ww = (double)SW;         // what _src gathers, and at most what _win_dev does
    if (kind == REMAP_WIN) {                                             // the window in host memory: read and checked during the call
        y0 = window[0]; x0 = window[1]; wh = window[2]; ww = window[3];
        SN_REQUIRE(std::isfinite(y0) && std::isfinite(x0) && std::isfinite(wh) && std::isfinite(ww),
                   "%s: window (%g, %g, %g, %g) is not finite", who, y0, x0, wh, ww);
        SN_REQUIRE(wh > 0.0 && ww > 0.0, "%s: window %g x %g is empty", who, wh, ww);
        // (a centred ratio window may overshoot by a rounding error; the taps clamp at the border anyway)
        SN_REQUIRE(y0 >= -1e-6 && x0 >= -1e-6 && y0 + wh <= (double)SH + 1e-6 && x0 + ww <= (double)SW + 1e-6,
                   "%s: window (%g, %g, %g, %g) leaves the %dx%d frame", who, y0, x0, wh, ww, SH, SW);
    }
    hipStream_t st = (hipStream_t)stream; Prof* prof = static_cast<Prof*>(profp);
    int rc = sn_check_device(src, nm.src, st);
    if (rc == 0) rc = sn_check_device(out, nm.out, st);
    if (rc == 0) rc = sn_check_device(workspace, nm.workspace, st);
    if (rc == 0 && kind == REMAP_WIN_DEV) rc = sn_check_device(window, nm.window, st);
    if (rc) return rc;
    const int h = H / rate, w = W / rate;
    rc = remap_shrink(x_map, y_map, N, H, W, h, w, workspace, st, prof);
    if (rc) return rc;
    WinRemapArgs wa;
    src_remap_args(wa.a, SH, SW, C, H, W, h, w, row_stride_bytes);
    wa.OH = OH; wa.OW = OW; wa.ws = {x0, y0, ww / (double)OW, wh / (double)OH};      // (_win_dev: not read, its kernels load the window)
    // algorithmic bytes: the window of the frame gathered once (_win_dev: not known here, at most the whole frame), the output written
    // once, the two small maps
    const double bytes = (double)N * ((wh * ww + (double)OH * OW) * C + 8.0 * h * w);
    const bool v4 = remap_vec4(C, OW, out, px_out, py_out);
    const int items = v4 ? OW / 4 : OW, threads = items >= 256 ? 256 : ((items + 63) & ~63);      // whole waves, a row segment each
    const dim3 grid(cdiv(items, threads), OH, N);
    static const struct { int id; const char* name; } kernels[3][2] = {
        {{PK_KERNEL_REMAP_SRC, "remap_src_kernel"}, {PK_KERNEL_REMAP_SRC4, "remap_src4_kernel"}},
        {{PK_KERNEL_REMAP_WIN, "remap_win_kernel"}, {PK_KERNEL_REMAP_WIN4, "remap_win4_kernel"}},
        {{PK_KERNEL_REMAP_WIN_DEV, "remap_win_dev_kernel"}, {PK_KERNEL_REMAP_WIN4_DEV, "remap_win4_dev_kernel"}}};
    if (cubic) {
        static const char* const cubic_names[3][2] = {{"remap_cubic_kernel<1, 0>", "remap_cubic_kernel<4, 0>"},
                                                      {"remap_cubic_kernel<1, 1>", "remap_cubic_kernel<4, 1>"},
                                                      {"remap_cubic_kernel<1, 2>", "remap_cubic_kernel<4, 2>"}};
        const double* dwin = kind == REMAP_WIN_DEV ? window : nullptr;      // (a host window is in wa.ws)
        const bool rec = prof && prof->begin(st);
        if (kind == REMAP_SRC) {
            if (v4) remap_cubic_kernel<4, 0><<<grid, threads, 0, st>>>(src, wa, dwin, workspace, out, black_count, px_out, py_out);
            else remap_cubic_kernel<1, 0><<<grid, threads, 0, st>>>(src, wa, dwin, workspace, out, black_count, px_out, py_out);
        } else if (kind == REMAP_WIN) {
            if (v4) remap_cubic_kernel<4, 1><<<grid, threads, 0, st>>>(src, wa, dwin, workspace, out, black_count, px_out, py_out);
            else remap_cubic_kernel<1, 1><<<grid, threads, 0, st>>>(src, wa, dwin, workspace, out, black_count, px_out, py_out);
        } else {
            if (v4) remap_cubic_kernel<4, 2><<<grid, threads, 0, st>>>(src, wa, dwin, workspace, out, black_count, px_out, py_out);
            else remap_cubic_kernel<1, 2><<<grid, threads, 0, st>>>(src, wa, dwin, workspace, out, black_count, px_out, py_out);
        }
        if (rec) prof->end(st, PK_KERNEL_REMAP_CUBIC + 2 * kind + (v4 ? 1 : 0), 0.0, bytes);
        SN_LAUNCH_CHECK(cubic_names[kind][v4]);
        return STABNET_OK;
    }
    const bool rec = prof && prof->begin(st);
    if (kind == REMAP_SRC) {
        if (v4) remap_src4_kernel<<<grid, threads, 0, st>>>(src, wa.a, workspace, out, black_count, px_out, py_out);
        else remap_src_kernel<<<grid, threads, 0, st>>>(src, wa.a, workspace, out, black_count, px_out, py_out);
    } else if (kind == REMAP_WIN) {
        if (v4) remap_win4_kernel<<<grid, threads, 0, st>>>(src, wa, workspace, out, black_count, px_out, py_out);
        else remap_win_kernel<<<grid, threads, 0, st>>>(src, wa, workspace, out, black_count, px_out, py_out);
    } else {
        if (v4) remap_win4_dev_kernel<<<grid, threads, 0, st>>>(src, wa, window, workspace, out, black_count, px_out, py_out);
        else remap_win_dev_kernel<<<grid, threads, 0, st>>>(src, wa, window, workspace, out, black_count, px_out, py_out);
    }
    if (rec) prof->end(st, kernels[kind][v4].id, 0.0, bytes);
    SN_LAUNCH_CHECK(kernels[kind][v4].name);
    return STABNET_OK;
}

// stabnet_warp_rev_bundle2_i420 and _i420_cubic: one entry, the kernel apart
static int remap_i420_entry(bool cubic, const unsigned char* src, int N, int SH, int SW, int planes, size_t frame_stride_bytes, const float* x_map,
        const float* y_map, int H, int W, int rate, const double* window, int OH, int OW, int border_y, unsigned char* out, int* black_count,
        float* workspace, void* stream, void* profp) {
    const char* who = cubic ? "warp_rev_bundle2_i420_cubic" : "warp_rev_bundle2_i420";
    SN_REQUIRE(src && x_map && y_map && out && workspace, "%s: null pointer", who);
    SN_REQUIRE(planes == 1 || planes == 3, "%s: planes must be 1 (Y only) or 3 (Y, U, V of a 4:2:0 frame), got %d", who, planes);
    SN_REQUIRE(N >= 1 && N <= 65535, "%s: batch %d outside 1..65535", who, N);
    SN_REQUIRE(SH >= 1 && SH <= 32767 && SW >= 1 && SW <= 32767, "%s: source %dx%d outside 1..32767 (the remap's 16-bit pixel index)", who, SH, SW);
    SN_REQUIRE(OH >= 1 && OH <= 32767 && OW >= 1 && OW <= 32767, "%s: output %dx%d outside 1..32767", who, OH, OW);
    SN_REQUIRE(planes == 1 || ((SH | SW | OH | OW) & 1) == 0, "%s: a 4:2:0 frame has even sides, got source %dx%d, output %dx%d", who, SH, SW, OH, OW);
    const size_t src_y = (size_t)SH * SW, src_c = planes == 3 ? (size_t)(SH / 2) * (SW / 2) : 0, src_bytes = src_y + 2 * src_c;
    SN_REQUIRE(frame_stride_bytes >= src_bytes, "%s: frame stride %zu < the frame's %zu bytes", who, frame_stride_bytes, src_bytes);
    SN_REQUIRE(border_y >= 0 && border_y <= 255, "%s: border_y %d outside 0..255", who, border_y);
    SN_REQUIRE(H >= 1 && W >= 1 && rate >= 1 && H / rate >= 1 && W / rate >= 1, "%s: maps %dx%d leave nothing at rate %d", who, H, W, rate);
    double y0 = 0.0, x0 = 0.0, wh = (double)SH, ww = (double)SW;
    if (window == nullptr) {
        SN_REQUIRE(OH == SH && OW == SW, "%s: a null window is the whole frame at its own size, got output %dx%d of source %dx%d", who, OH, OW, SH, SW);
    } else {
        y0 = window[0]; x0 = window[1]; wh = window[2]; ww = window[3];
        SN_REQUIRE(std::isfinite(y0) && std::isfinite(x0) && std::isfinite(wh) && std::isfinite(ww),
                   "%s: window (%g, %g, %g, %g) is not finite", who, y0, x0, wh, ww);
        SN_REQUIRE(wh > 0.0 && ww > 0.0, "%s: window %g x %g is empty", who, wh, ww);
        SN_REQUIRE(y0 >= -1e-6 && x0 >= -1e-6 && y0 + wh <= (double)SH + 1e-6 && x0 + ww <= (double)SW + 1e-6,
                   "%s: window (%g, %g, %g, %g) leaves the %dx%d frame", who, y0, x0, wh, ww, SH, SW);
    }
    hipStream_t st = (hipStream_t)stream; Prof* prof = static_cast<Prof*>(profp);
    int rc = sn_check_device(src, cubic ? "warp_rev_bundle2_i420_cubic: src" : "warp_rev_bundle2_i420: src", st);
    if (rc == 0) rc = sn_check_device(out, cubic ? "warp_rev_bundle2_i420_cubic: out" : "warp_rev_bundle2_i420: out", st);
    if (rc == 0) rc = sn_check_device(workspace, cubic ? "warp_rev_bundle2_i420_cubic: workspace" : "warp_rev_bundle2_i420: workspace", st);
    if (rc) return rc;
    const int h = H / rate, w = W / rate;
    rc = remap_shrink(x_map, y_map, N, H, W, h, w, workspace, st, prof);
    if (rc) return rc;
    I420Args ia;
    const size_t out_y = (size_t)OH * OW, out_c = planes == 3 ? (size_t)(OH / 2) * (OW / 2) : 0;
    ia.src_frame = frame_stride_bytes; ia.out_frame = out_y + 2 * out_c;
    ia.src_off[0] = 0; ia.src_off[1] = src_y; ia.src_off[2] = src_y + src_c;
    ia.out_off[0] = 0; ia.out_off[1] = out_y; ia.out_off[2] = out_y + out_c;
    ia.border[0] = border_y; ia.border[1] = 128; ia.border[2] = 128;
    int items = 0;
    for (int k = 0; k < 2; ++k) {                            // luma; chroma: every length and the window halved (exact)
        const int d = k + 1;
        if (k == 1 && planes == 1) { ia.g[1] = ia.g[0]; ia.g[1].OH = 0; break; }
        I420Geom& g = ia.g[k];
        src_remap_args(g.a, SH / d, SW / d, 1, H, W, h, w, (size_t)(SW / d));
        g.OH = OH / d; g.OW = OW / d;
        g.ws = {x0 / d, y0 / d, (ww / d) / (double)g.OW, (wh / d) / (double)g.OH};
    }
    for (int p = 0; p < 3; ++p) {
        const I420Geom& g = ia.g[p != 0];
        const bool aligned = (((size_t)out + ia.out_off[p]) & 3) == 0 && (N == 1 || (ia.out_frame & 3) == 0);
        ia.px4[p] = (p < planes && remap_vec4_enabled() && g.OW % 4 == 0 && aligned) ? 1 : 0;
        if (p < planes && (ia.px4[p] ? g.OW / 4 : g.OW) > items) items = ia.px4[p] ? g.OW / 4 : g.OW;
    }
    const int threads = items >= 256 ? 256 : ((items + 63) & ~63);       // whole waves, a row segment each
    const dim3 grid(cdiv(items, threads), ia.g[0].OH + (planes == 3 ? 2 * ia.g[1].OH : 0), N);
    // algorithmic bytes: the window of every plane gathered once, the output written once, the two small maps
    const double cf = planes == 3 ? 1.5 : 1.0, bytes = (double)N * ((wh * ww + (double)OH * OW) * cf + 8.0 * h * w);
    const bool rec = prof && prof->begin(st);
    if (cubic) remap_i420_kernel<true><<<grid, threads, 0, st>>>(src, ia, workspace, out, black_count);
    else remap_i420_kernel<false><<<grid, threads, 0, st>>>(src, ia, workspace, out, black_count);
    if (rec) prof->end(st, cubic ? PK_KERNEL_REMAP_I420_CUBIC : PK_KERNEL_REMAP_I420, 0.0, bytes);
    SN_LAUNCH_CHECK(cubic ? "remap_i420_kernel<true>" : "remap_i420_kernel");
    return STABNET_OK;
}

extern "C" {

/* warpRevBundle2(img, x_map, y_map) (deploy_bundle.py:136-146): img uint8 [N,H,W,C] (BGR, C = 3), x_map, y_map [N,H,W]
 * normalised (the warp's outputs) -> out uint8 [N,H,W,C].  workspace: 2*N*(H/rate)*(W/rate) floats.  px_out/py_out
 * (optional, [N,H,W]): the smoothed maps in pixel coordinates that cv2.remap would receive. */
int stabnet_warp_rev_bundle2(const unsigned char* img, const float* x_map, const float* y_map, int N, int H, int W, int C,
                             int rate, unsigned char* out, float* workspace, float* px_out, float* py_out, void* stream) {
    SN_REQUIRE(img && x_map && y_map && out && workspace, "warp_rev_bundle2: null pointer");
    SN_REQUIRE(N > 0 && N <= 65535 && C > 0 && rate >= 1 && H / rate >= 1 && W / rate >= 1, "warp_rev_bundle2: bad shape");
    SN_REQUIRE((px_out == nullptr) == (py_out == nullptr), "warp_rev_bundle2: px_out and py_out go together");
    const int h = H / rate, w = W / rate;
    hipStream_t st = (hipStream_t)stream;
    const int rc = remap_shrink(x_map, y_map, N, H, W, h, w, workspace, st, nullptr);
    if (rc) return rc;
    SrcRemapArgs a;                                          // the source is the network-size frame itself, dense
    src_remap_args(a, H, W, C, H, W, h, w, (size_t)W * C);
    // (W % 4 == 0 makes the frame at least 12 bytes: the loader's first tap is always inside it)
    if (remap_vec4(C, W, out, px_out, py_out) && ((size_t)img & 3) == 0) {
        remap_color4_kernel<<<dim3(cdiv((long)H * W / 4, 256), N), 256, 0, st>>>(img, a, workspace, out, px_out, py_out);
        SN_LAUNCH_CHECK("remap_color4_kernel");
        return STABNET_OK;
    }
    remap_color_kernel<<<dim3(cdiv((long)H * W, 256), N), 256, 0, st>>>(img, a, workspace, out, px_out, py_out);
    SN_LAUNCH_CHECK("remap_color_kernel");
    return STABNET_OK;
}

/* warpRevBundle2 at SOURCE resolution: src uint8 [N,SH,SW,C] (rows row_stride_bytes apart) remapped by the network-size maps
 * x_map, y_map [N,H,W] -> out uint8 [N,SH,SW,C] dense.  black_count (optional, int32 [N,SH,SW]): += 1 on pixels whose rounded
 * coordinate lies outside the frame.  px_out/py_out (optional, [N,SH,SW]): the source-pixel coordinates cv2.remap would receive. */
int stabnet_warp_rev_bundle2_src(const unsigned char* src, int N, int SH, int SW, int C, size_t row_stride_bytes, const float* x_map,
        const float* y_map, int H, int W, int rate, unsigned char* out, int* black_count, float* workspace, float* px_out, float* py_out,
        void* stream, void* profp) {
    return remap_src_entry(REMAP_SRC, false, src, N, SH, SW, C, row_stride_bytes, x_map, y_map, H, W, rate, nullptr, SH, SW, out, black_count, workspace,
                           px_out, py_out, stream, profp);
}

/* stabnet_warp_rev_bundle2_src through a window of the stabilised frame: out uint8 [N,OH,OW,C] dense, output pixel (i, j) = the
 * stabilised frame at SH x SW sampled at the fractional position inside window = {y0, x0, wh, ww} (host memory, pixel-edge units,
 * read during the call).  black_count, px_out/py_out: [N,OH,OW], at the OUTPUT pixel. */
int stabnet_warp_rev_bundle2_win(const unsigned char* src, int N, int SH, int SW, int C, size_t row_stride_bytes, const float* x_map,
        const float* y_map, int H, int W, int rate, const double* window, int OH, int OW, unsigned char* out, int* black_count,
        float* workspace, float* px_out, float* py_out, void* stream, void* profp) {
    return remap_src_entry(REMAP_WIN, false, src, N, SH, SW, C, row_stride_bytes, x_map, y_map, H, W, rate, window, OH, OW, out, black_count, workspace,
                           px_out, py_out, stream, profp);
}

/* stabnet_warp_rev_bundle2_win with the window in DEVICE memory: window double [N,4] = {y0, x0, wh, ww} per stream, read by the
 * kernels when they run -- what an earlier launch on the stream (stabnet_fill_window_update) wrote is what they see, also when the
 * launches are replayed from a captured graph.  A window whose values _win would refuse gives the whole frame. */
int stabnet_warp_rev_bundle2_win_dev(const unsigned char* src, int N, int SH, int SW, int C, size_t row_stride_bytes, const float* x_map,
        const float* y_map, int H, int W, int rate, const double* window, int OH, int OW, unsigned char* out, int* black_count,
        float* workspace, float* px_out, float* py_out, void* stream, void* profp) {
    return remap_src_entry(REMAP_WIN_DEV, false, src, N, SH, SW, C, row_stride_bytes, x_map, y_map, H, W, rate, window, OH, OW, out, black_count, workspace,
                           px_out, py_out, stream, profp);
}

/* stabnet_warp_rev_bundle2_win of a planar 4:2:0 frame (remap_i420_kernel above): src N frames frame_stride_bytes apart, each the Y plane
 * [SH,SW] and, with planes == 3, U and V [SH/2,SW/2] behind it, dense, any base alignment; out the same layout at OH x OW, dense.
 * window {y0, x0, wh, ww} in HOST memory, in pixel-edge units of the stabilised LUMA frame (null: the whole frame, OH, OW == SH, SW); a
 * chroma plane goes through the halved window.  Taps outside a plane read border_y (Y) or 128 (U, V).  black_count (optional, int32
 * [N,OH,OW]): at the luma output pixel.  Two launches: the shrink, then one gather over every plane of every frame. */
int stabnet_warp_rev_bundle2_i420(const unsigned char* src, int N, int SH, int SW, int planes, size_t frame_stride_bytes, const float* x_map,
        const float* y_map, int H, int W, int rate, const double* window, int OH, int OW, int border_y, unsigned char* out, int* black_count,
        float* workspace, void* stream, void* profp) {
    return remap_i420_entry(false, src, N, SH, SW, planes, frame_stride_bytes, x_map, y_map, H, W, rate, window, OH, OW, border_y, out, black_count,
                            workspace, stream, profp);
}

/* The remaps above with cv2.remap's INTER_CUBIC in place of INTER_LINEAR (remap_cubic_kernel<PX, KIND>): 16 taps per channel at rows
 * iy - 1 .. iy + 2, columns ix - 1 .. ix + 2, OpenCV's 15-bit table weights (g_cubic_tab through cubic_weights), out = clamp((sum +
 * 16384) >> 15).  window_kind 0: the whole frame at its own size (window not read; OH, OW == SH, SW; with SH, SW == H, W the
 * network-size remap), 1: window = four doubles in host memory, 2: window double [N,4] in device memory.  Coordinates, coverage and
 * every refusal are the bilinear entries'. */
int stabnet_warp_rev_bundle2_cubic(const unsigned char* src, int N, int SH, int SW, int C, size_t row_stride_bytes, const float* x_map,
        const float* y_map, int H, int W, int rate, int window_kind, const double* window, int OH, int OW, unsigned char* out, int* black_count,
        float* workspace, float* px_out, float* py_out, void* stream, void* profp) {
    SN_REQUIRE(window_kind >= 0 && window_kind <= 2, "warp_rev_bundle2_cubic: window_kind must be 0 (none), 1 (host) or 2 (device), got %d", window_kind);
    const RemapKind kind = window_kind == 0 ? REMAP_SRC : (window_kind == 1 ? REMAP_WIN : REMAP_WIN_DEV);
    return remap_src_entry(kind, true, src, N, SH, SW, C, row_stride_bytes, x_map, y_map, H, W, rate, window, OH, OW, out, black_count, workspace,
                           px_out, py_out, stream, profp);
}

/* stabnet_warp_rev_bundle2_i420 with the bicubic taps on every plane (remap_i420_kernel<true>); taps outside a plane read border_y / 128. */
int stabnet_warp_rev_bundle2_i420_cubic(const unsigned char* src, int N, int SH, int SW, int planes, size_t frame_stride_bytes, const float* x_map,
        const float* y_map, int H, int W, int rate, const double* window, int OH, int OW, int border_y, unsigned char* out, int* black_count,
        float* workspace, void* stream, void* profp) {
    return remap_i420_entry(true, src, N, SH, SW, planes, frame_stride_bytes, x_map, y_map, H, W, rate, window, OH, OW, border_y, out, black_count,
                            workspace, stream, profp);
}

/* BicubicTab_i by the functions the kernels' table is compiled from, run on the host (no GPU): out short [1024][16], entry fy * 32 + fx,
 * tap k1 * 4 + k2. */
int stabnet_remap_cubic_table(short* out) {
    SN_REQUIRE(out != nullptr, "remap_cubic_table: null pointer");
    for (int e = 0; e < 1024; ++e) {
        int w[16];
        cubic_weights_calc(e & 31, e >> 5, w);               // evaluated here, at run time: not a copy of the compiled table
        for (int k = 0; k < 16; ++k) out[e * 16 + k] = (short)w[k];
    }
    return STABNET_OK;
}

/* The same 16384 values written by the device, each phase through the function the remap kernels call (a read of their table): one launch. */
int stabnet_remap_cubic_weights_dev(short* out_dev, void* stream) {
    SN_REQUIRE(out_dev != nullptr, "remap_cubic_weights_dev: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int rc = sn_check_device(out_dev, "remap_cubic_weights_dev: out", st);
    if (rc) return rc;
    remap_cubic_weights_kernel<<<4, 256, 0, st>>>(out_dev);
    SN_LAUNCH_CHECK("remap_cubic_weights_kernel");
    return STABNET_OK;
}

/* The adaptive window of one frame per stream (fill_window_kernel above): x_map, y_map [N,H,W] as the remap receives them; state
 * double [N] (the ratio of the previous frame, 1.0 at the start of a clip), window double [N,4], stats int32 [N,2] = {key, bad nodes},
 * workspace 2*N*h*w floats, all in device memory.  Two launches: the shrink, then one workgroup per stream. */
int stabnet_fill_window_update(const float* x_map, const float* y_map, int N, int H, int W, int rate, int SH, int SW,
                               double r_min, double up, int margin_q, double* state, double* window, int* stats,
                               float* workspace, void* stream) {
    SN_REQUIRE(x_map && y_map && state && window && stats && workspace, "fill_window_update: null pointer");
    SN_REQUIRE(N >= 1 && N <= 65535, "fill_window_update: batch %d outside 1..65535", N);
    SN_REQUIRE(SH >= 1 && SH <= 32767 && SW >= 1 && SW <= 32767,
               "fill_window_update: source %dx%d outside 1..32767 (the remap's 16-bit pixel index)", SH, SW);
    SN_REQUIRE(H >= 1 && W >= 1 && rate >= 1 && H / rate >= 1 && W / rate >= 1, "fill_window_update: maps %dx%d leave nothing at rate %d", H, W, rate);
    SN_REQUIRE((long)(H / rate) * (W / rate) <= (1L << 30), "fill_window_update: %ld nodes overflow the int32 key", (long)(H / rate) * (W / rate));
    SN_REQUIRE(r_min > 0.0 && r_min <= 1.0, "fill_window_update: r_min %g outside (0, 1]", r_min);
    SN_REQUIRE(std::isfinite(up) && up >= 0.0, "fill_window_update: up %g must be finite and >= 0", up);
    SN_REQUIRE(margin_q >= 0 && margin_q <= 16 * (SH < SW ? SH : SW), "fill_window_update: margin_q %d outside 0..16 * min(%d, %d)", margin_q, SH, SW);
    const int h = H / rate, w = W / rate;
    hipStream_t st = (hipStream_t)stream;
    int rc = sn_check_device(state, "fill_window_update: state", st);
    if (rc == 0) rc = sn_check_device(window, "fill_window_update: window", st);
    if (rc == 0) rc = sn_check_device(stats, "fill_window_update: stats", st);
    if (rc == 0) rc = sn_check_device(workspace, "fill_window_update: workspace", st);
    if (rc) return rc;
    rc = remap_shrink(x_map, y_map, N, H, W, h, w, workspace, st, nullptr);
    if (rc) return rc;
    FillArgs fa;
    src_remap_args(fa.a, SH, SW, 1, H, W, h, w, (size_t)SW);
    fa.margin_q = margin_q; fa.r_min = r_min; fa.up = up;
    const int nodes = h * w, threads = nodes >= 1024 ? 1024 : ((nodes + 63) & ~63);
    fill_window_kernel<<<N, threads, 0, st>>>(workspace, fa, state, window, stats);
    SN_LAUNCH_CHECK("fill_window_kernel");
    return STABNET_OK;
}

/* cvt_train2img (deploy_bundle.py:75): out[i] = uint8((x[i] + 0.5) * 255), clipped to [0, 255].  x float [n], out uint8 [n]. */
int stabnet_cvt_train2img(const float* x, unsigned char* out, long n, void* stream) {
    SN_REQUIRE(x && out && n > 0, "cvt_train2img: bad arguments");
    cvt_train2img_kernel<<<cdiv(cdiv(n, 4), 256), 256, 0, (hipStream_t)stream>>>(x, out, n);
    SN_LAUNCH_CHECK("cvt_train2img_kernel");
    return STABNET_OK;
}

}  // extern "C"
