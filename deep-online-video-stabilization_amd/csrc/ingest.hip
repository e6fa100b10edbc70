// Frame ingest (config.py:6-21 cvt_img2train; deploy_bundle.py:215,303 cv2.resize): a uint8 frame of any size, as read from the
// video, to the network's grey input and the network-size colour frame, on the device.
//   ingest_grey_rows_kernel : one workgroup per (source row, tile of output columns): the row's bytes -> LDS as aligned dwords,
//                             BGR -> grey (cv2.cvtColor fixed point, 8 bits) in LDS, Pillow's horizontal BILINEAR pass, ROUNDED AND
//                             CLIPPED TO 8 BITS, -> workspace uint8 [N][rows the vertical pass reads][W]
//   ingest_grey_cols_kernel : one lane per output pixel: Pillow's vertical pass over the workspace, 8 bits, then the 256-entry table
//                             float32(float64(u) * (1./255) - 0.5) built by the host -> float32 [N][H][W]
//   ingest_colour_kernel    : one workgroup per (output row, tile of output columns): the two source rows -> LDS as aligned dwords,
//                             cv2.resize INTER_LINEAR's 11-bit fixed point, one lane per output byte, no intermediate
// Pillow's filter is a triangle whose support grows with the downscale factor; the tap tables (bounds + 22-bit coefficients per
// output, stabnet_ingest_pil_taps) and cv2's (two offsets + two 11-bit coefficients, stabnet_ingest_cv_taps) are built once per
// geometry by the host functions below and live on the device.  Nothing allocates, synchronises or copies from the host inside
// the two entry points, and their arguments are fixed per geometry, so the launches can sit in a captured frame graph.
// [external] The grey conversion and the colour resize restate OpenCV's published arithmetic (cv2 is not a dependency), as
// remap.hip does; the Pillow resize is pinned bit for bit by the installed Pillow (tests/test_ingest_*.py).
#include <cmath>
#include <vector>
#include "common.h"
#include "prof.h"

namespace {

constexpr int kPilBits = 22;             // Pillow's PRECISION_BITS
constexpr int kMaxTaps = 8193;           // horizontal taps of the grey path: the span of ONE output must fit the LDS tile (4096x downscale)
constexpr int kSpanCap = 12288;          // source pixels of one tile: 3 B raw + 1 B grey each = 48 KB of LDS
constexpr int kTileCap = 4096;           // output columns of one tile
constexpr int kThreads = 256;

// Bytes [g, g + nbytes) -> LDS at the same position modulo 4, so that every dword that lies wholly inside the range is ONE aligned
// dword load and ONE aligned LDS store; the (up to 3 + 3) bytes in front of the first and behind the last such dword go as bytes.
// Nothing outside [g, g + nbytes) is read: any base pointer and any row stride are accepted (.npy rows of odd width are not
// dword-aligned).  Returns the offset of byte g[0] in `lds` (0..3).
__device__ __forceinline__ int stage_bytes(const unsigned char* __restrict__ g, long nbytes, unsigned int* lds) {
    const int m = (int)((uintptr_t)g & 3);
    unsigned char* lb = reinterpret_cast<unsigned char*>(lds);
    const long head = (m ? 4 - m : 0) < nbytes ? (m ? 4 - m : 0) : nbytes;
    const long nd = (nbytes - head) >> 2;
    const unsigned int* gd = reinterpret_cast<const unsigned int*>(g + head);
    unsigned int* ld = lds + ((m + head) >> 2);
    for (long i = threadIdx.x; i < nd; i += blockDim.x) ld[i] = gd[i];
    const long tail0 = head + 4 * nd;
    if ((long)threadIdx.x < head) lb[m + threadIdx.x] = g[threadIdx.x];
    if ((long)threadIdx.x < nbytes - tail0) lb[m + tail0 + threadIdx.x] = g[tail0 + threadIdx.x];
    return m;
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// grid (source rows needed, column tiles, N).  xb / xk == NULL: no horizontal pass (rw == sw), the window's columns are copied.
__global__ __launch_bounds__(kThreads) void ingest_grey_rows_kernel(const unsigned char* __restrict__ img, size_t frame_stride, size_t row_stride,
                                                                     int C, int wb, int wg, int wr, int shift, int r0, int dx, int W, int tile,
                                                                     const int* __restrict__ xb, const int* __restrict__ xk, int kx,
                                                                     unsigned char* __restrict__ tmp, int nrows) {
    extern __shared__ unsigned int lds[];
    const int row = blockIdx.x, n = blockIdx.z;
    const int o0 = blockIdx.y * tile, o1 = min(o0 + tile, W);                 // outputs [o0, o1) of the window
    int lo, hi;                                                              // source pixels [lo, hi) this tile reads
    if (xb) { lo = xb[2 * (dx + o0)]; hi = xb[2 * (dx + o1 - 1)] + xb[2 * (dx + o1 - 1) + 1]; }
    else    { lo = dx + o0; hi = dx + o1; }
    const int span = hi - lo;
    const unsigned char* g = img + (size_t)n * frame_stride + (size_t)(r0 + row) * row_stride + (size_t)lo * C;
    const int m = stage_bytes(g, (long)span * C, lds);
    const unsigned char* raw = reinterpret_cast<const unsigned char*>(lds) + m;
    const unsigned char* grey = raw;
    if (C == 3) {
        // cv2.cvtColor(BGR2GRAY), uint8: fixed point, rounded to 8 bits
        unsigned char* gl = reinterpret_cast<unsigned char*>(lds) + (((size_t)span * 3 + 3 + 3) & ~(size_t)3);
        __syncthreads();
        const int half = 1 << (shift - 1);
        for (int i = threadIdx.x; i < span; i += blockDim.x)
            gl[i] = (unsigned char)((raw[3 * i] * wb + raw[3 * i + 1] * wg + raw[3 * i + 2] * wr + half) >> shift);
        grey = gl;
    }
    __syncthreads();
    unsigned char* out = tmp + ((size_t)n * nrows + row) * W;
    for (int o = o0 + threadIdx.x; o < o1; o += blockDim.x) {
        int v;
        if (xb) {
            const int xmin = xb[2 * (dx + o)], cnt = xb[2 * (dx + o) + 1];
            const int* k = xk + (size_t)(dx + o) * kx;
            const unsigned char* s = grey + (xmin - lo);
            int acc = 1 << (kPilBits - 1);
            for (int t = 0; t < cnt; ++t) acc += (int)s[t] * k[t];
            v = clip8(acc >> kPilBits);                                      // Pillow's 8-bit intermediate
        } else {
            v = grey[o - o0];
        }
        out[o] = (unsigned char)v;
    }
}

// grid (cdiv(W, 256), H, N).  yb / yk == NULL: no vertical pass (rh == sh), tmp row y is window row y.
__global__ __launch_bounds__(kThreads) void ingest_grey_cols_kernel(const unsigned char* __restrict__ tmp, int nrows, int r0, int dy, int H, int W,
                                                                     const int* __restrict__ yb, const int* __restrict__ yk, int ky,
                                                                     const float* __restrict__ lut, float* __restrict__ out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
    if (x >= W) return;
    const unsigned char* t = tmp + (size_t)n * nrows * W + x;
    int u;
    if (yb) {
        const int ymin = yb[2 * (dy + y)], cnt = yb[2 * (dy + y) + 1];
        const int* k = yk + (size_t)(dy + y) * ky;
        const unsigned char* s = t + (size_t)(ymin - r0) * W;
        int acc = 1 << (kPilBits - 1);
        for (int i = 0; i < cnt; ++i) acc += (int)s[(size_t)i * W] * k[i];
        u = clip8(acc >> kPilBits);
    } else {
        u = t[(size_t)y * W];
    }
    out[((size_t)n * H + y) * W + x] = lut[u];                               // float32(float64(u) * (1./255) - 0.5), from the host
}

// grid (H, column tiles, N).  cv2.resize(INTER_LINEAR) of uint8 [sh, sw, C]: xo / yo [dst][2] source indices, xc / yc [dst][2]
// coefficients of 2048.
__global__ __launch_bounds__(kThreads) void ingest_colour_kernel(const unsigned char* __restrict__ img, size_t frame_stride, size_t row_stride,
                                                                  int C, int H, int W, int tile, const int* __restrict__ xo,
                                                                  const short* __restrict__ xc, const int* __restrict__ yo,
                                                                  const short* __restrict__ yc, unsigned char* __restrict__ out) {
    extern __shared__ unsigned int lds[];
    const int y = blockIdx.x, n = blockIdx.z;
    const int o0 = blockIdx.y * tile, o1 = min(o0 + tile, W);
    const int lo = xo[2 * o0], hi = xo[2 * (o1 - 1) + 1] + 1;
    const long nbytes = (long)(hi - lo) * C;
    const size_t half = ((size_t)nbytes + 3 + 3) >> 2;                       // dwords of one staged row
    const unsigned char* f = img + (size_t)n * frame_stride + (size_t)lo * C;
    const int y0 = yo[2 * y], y1 = yo[2 * y + 1];
    const int m = stage_bytes(f + (size_t)y0 * row_stride, nbytes, lds);
    const int m1 = stage_bytes(f + (size_t)y1 * row_stride, nbytes, lds + half);
    const unsigned char* a = reinterpret_cast<const unsigned char*>(lds) + m;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(lds + half) + m1;
    __syncthreads();
    const int b0 = yc[2 * y], b1 = yc[2 * y + 1];
    unsigned char* o = out + (((size_t)n * H + y) * W + o0) * C;
    const int nout = (o1 - o0) * C;
    for (int j = threadIdx.x; j < nout; j += blockDim.x) {
        const int xx = o0 + j / C, c = j % C;
        const int p0 = (xo[2 * xx] - lo) * C + c, p1 = (xo[2 * xx + 1] - lo) * C + c;
        const int a0 = xc[2 * xx], a1 = xc[2 * xx + 1];
        const int s0 = a[p0] * a0 + a[p1] * a1, s1 = b[p0] * a0 + b[p1] * a1;
        o[j] = (unsigned char)((((b0 * (s0 >> 4)) >> 16) + ((b1 * (s1 >> 4)) >> 16) + 2) >> 2);
    }
}

// Pillow's bounds of output i of one axis (Resample.c precompute_coeffs), in double as Pillow computes them.
void pil_bounds(int in, int out, int i, int* xmin, int* xmax) {
    const double scale = (double)in / (double)out, support = scale < 1.0 ? 1.0 : scale;
    const double center = (i + 0.5) * scale;
    int lo = (int)(center - support + 0.5), hi = (int)(center + support + 0.5);
    *xmin = lo < 0 ? 0 : lo;
    *xmax = hi > in ? in : hi;
}

int pil_ksize(int in, int out) {
    const double scale = (double)in / (double)out;
    return (int)std::ceil(scale < 1.0 ? 1.0 : scale) * 2 + 1;
}

// Output columns per tile such that the source span of a tile stays within `cap` pixels: span <= (tile - 1) * scale + reach.
int tile_of(int W, double scale, double reach, int cap) {
    double t = ((double)cap - reach) / scale + 1.0;
    if (t < 1.0) t = 1.0;
    if (t > (double)kTileCap) t = kTileCap;
    const int tile = (int)t;
    return tile < W ? tile : W;
}

struct GreyGeom { int r0, nrows; };      // source rows [r0, r0 + nrows) that the window's vertical pass reads

bool grey_geom(int sh, int sw, int C, int rh, int rw, int dy, int dx, int H, int W, GreyGeom* g) {
    if (sh < 1 || sw < 1 || (C != 1 && C != 3) || rh < 1 || rw < 1 || H < 1 || W < 1 || dy < 0 || dx < 0) return false;
    if ((long)dy + H > rh || (long)dx + W > rw) return false;
    if (rh == sh) { g->r0 = dy; g->nrows = H; return true; }
    int lo, hi, t;
    pil_bounds(sh, rh, dy, &lo, &t);
    pil_bounds(sh, rh, dy + H - 1, &t, &hi);
    g->r0 = lo; g->nrows = hi - lo;
    return g->nrows >= 1;
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

/* Pillow's BILINEAR coefficients of one axis.  Returns out * ksize (the ints `kk` takes); with ksize / bounds2 / kk NULL only that.
 * bounds2 [out][2] = (first source sample, number of taps), kk [out][ksize] (unused taps 0). */
int stabnet_ingest_pil_taps(int in, int out, int* ksize, int* bounds2, int* kk, int cap) {
    SN_REQUIRE(in >= 1 && out >= 1, "ingest_pil_taps: sizes must be >= 1, got %d -> %d", in, out);
    const int ks = pil_ksize(in, out);
    SN_REQUIRE((long)out * ks <= 0x7fffffffL, "ingest_pil_taps: table of %d x %d taps is too large", out, ks);
    if (ksize) *ksize = ks;
    if (!bounds2 && !kk) return out * ks;
    SN_REQUIRE(bounds2 && kk, "ingest_pil_taps: null pointer");
    SN_REQUIRE(cap >= out * ks, "ingest_pil_taps: %d ints needed, cap is %d", out * ks, cap);
    const double scale = (double)in / (double)out, filterscale = scale < 1.0 ? 1.0 : scale;
    const double ss = 1.0 / filterscale;
    std::vector<double> k(ks);
    for (int i = 0; i < out; ++i) {
        const double center = (i + 0.5) * scale;
        int xmin, xmax;
        pil_bounds(in, out, i, &xmin, &xmax);
        const int n = xmax - xmin;
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            double a = (x + xmin - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            const double w = a < 1.0 ? 1.0 - a : 0.0;
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < ks; ++x) {
            double v = 0.0;
            if (x < n) v = ww != 0.0 ? k[x] / ww : k[x];
            kk[(size_t)i * ks + x] = (int)(0.5 + v * (double)(1 << kPilBits));
        }
        bounds2[2 * i] = xmin;
        bounds2[2 * i + 1] = n;
    }
    return out * ks;
}

/* cv2.resize INTER_LINEAR of one axis: ofs2 [dst][2] = the two source indices, coef2 [dst][2] = their weights of 2048. */
int stabnet_ingest_cv_taps(int src, int dst, int* ofs2, short* coef2) {
    SN_REQUIRE(src >= 1 && dst >= 1, "ingest_cv_taps: sizes must be >= 1, got %d -> %d", src, dst);
    SN_REQUIRE(ofs2 && coef2, "ingest_cv_taps: null pointer");
    const double scale = 1.0 / ((double)dst / (double)src);
    for (int d = 0; d < dst; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= (float)s;
        if (s < 0) { s = 0; f = 0.f; }
        if (s >= src - 1) { s = src - 1; f = 0.f; }
        ofs2[2 * d] = s;
        ofs2[2 * d + 1] = s + 1 < src ? s + 1 : src - 1;
        coef2[2 * d] = (short)std::nearbyint((1.f - f) * 2048.f);            // ties to even (the default rounding mode), as cvRound
        coef2[2 * d + 1] = (short)std::nearbyint(f * 2048.f);
    }
    return STABNET_OK;
}

/* Bytes of the 8-bit intermediate of stabnet_ingest_grey: N x (source rows the window's vertical pass reads) x W.  0 = bad arguments. */
size_t stabnet_ingest_workspace_bytes(int N, int sh, int sw, int C, int rh, int rw, int H, int W) {
    GreyGeom g;
    if (N < 1 || !grey_geom(sh, sw, C, rh, rw, 0, 0, H, W, &g)) {
        stabnet_set_error("ingest_workspace_bytes: bad batch, shape, channels or window");
        return 0;
    }
    // the window's origin is not an argument: wherever it lies, its first and last output read source rows less than
    // (H - 1) * scale + 2 * support + 1 apart (Pillow truncates both ends), and never more than the source has
    const double scale = (double)sh / (double)rh, span = (H - 1) * scale + 2.0 * (scale < 1.0 ? 1.0 : scale) + 2.0;
    const int rows = rh == sh ? H : (span < (double)sh ? (int)span : sh);
    return align16((size_t)N * rows * W);
}

int stabnet_ingest_grey(const unsigned char* img, int N, int sh, int sw, int C, size_t row_stride_bytes, int wb, int wg, int wr,
                        int shift, int rh, int rw, int dy, int dx, int H, int W, const int* xbounds_dev, const int* xkk_dev, int xksize,
                        const int* ybounds_dev, const int* ykk_dev, int yksize, const float* lut256_dev, float* out, void* workspace,
                        size_t workspace_bytes, void* stream, void* profp) {
    SN_REQUIRE(img && lut256_dev && out && workspace, "ingest_grey: null pointer");
    SN_REQUIRE(C == 1 || C == 3, "ingest_grey: C must be 1 (grey) or 3 (BGR), got %d", C);
    SN_REQUIRE(N >= 1 && N <= 65535 && sh >= 1 && sw >= 1 && rh >= 1 && rw >= 1 && H >= 1 && W >= 1,
               "ingest_grey: batch (1..65535) and every size must be >= 1");
    SN_REQUIRE(H <= 65535, "ingest_grey: H %d > 65535", H);
    SN_REQUIRE(row_stride_bytes >= (size_t)sw * C, "ingest_grey: row stride %zu < %d * %d bytes", row_stride_bytes, sw, C);
    SN_REQUIRE(shift >= 1 && shift <= 22 && wb >= 0 && wg >= 0 && wr >= 0 && (long)wb + wg + wr <= (1L << shift),
               "ingest_grey: grey weights must be >= 0 and sum to at most 1 << shift (1..22)");
    GreyGeom g;
    SN_REQUIRE(grey_geom(sh, sw, C, rh, rw, dy, dx, H, W, &g), "ingest_grey: window %dx%d at (%d, %d) lies outside the resize target %dx%d", H,
               W, dy, dx, rh, rw);
    const bool hpass = rw != sw, vpass = rh != sh;
    SN_REQUIRE(!hpass || (xbounds_dev && xkk_dev), "ingest_grey: null pointer (horizontal tap tables, %d -> %d)", sw, rw);
    SN_REQUIRE(!vpass || (ybounds_dev && ykk_dev), "ingest_grey: null pointer (vertical tap tables, %d -> %d)", sh, rh);
    SN_REQUIRE(!hpass || xksize == pil_ksize(sw, rw), "ingest_grey: xksize %d, stabnet_ingest_pil_taps gives %d for %d -> %d", xksize,
               pil_ksize(sw, rw), sw, rw);
    SN_REQUIRE(!vpass || yksize == pil_ksize(sh, rh), "ingest_grey: yksize %d, stabnet_ingest_pil_taps gives %d for %d -> %d", yksize,
               pil_ksize(sh, rh), sh, rh);
    SN_REQUIRE(!hpass || xksize <= kMaxTaps, "ingest_grey: %d horizontal taps, the kernel holds at most %d (a 4096x downscale)", xksize, kMaxTaps);
    const size_t need = (size_t)N * g.nrows * W;
    if (workspace_bytes < need) {
        stabnet_set_error("ingest_grey: workspace %zu < %zu bytes", workspace_bytes, need);
        return STABNET_ERR_WORKSPACE;
    }
    const double xscale = (double)sw / (double)rw;
    const int tile = hpass ? tile_of(W, xscale, 2.0 * (xscale < 1.0 ? 1.0 : xscale) + 3.0, kSpanCap) : (W < kTileCap ? W : kTileCap);
    const int tiles = cdiv(W, tile);
    SN_REQUIRE(tiles <= 65535, "ingest_grey: %d column tiles > 65535", tiles);
    hipStream_t st = (hipStream_t)stream;
    int rc = sn_check_device(img, "ingest_grey: img", st);
    if (rc == 0) rc = sn_check_device(out, "ingest_grey: out", st);
    if (rc == 0) rc = sn_check_device(workspace, "ingest_grey: workspace", st);
    if (rc) return rc;
    Prof* prof = static_cast<Prof*>(profp);
    unsigned char* tmp = static_cast<unsigned char*>(workspace);
    // LDS of a tile: its source span, raw (+ 3 bytes in front, rounded to dwords) and, for BGR, grey
    const long span = hpass ? (long)((tile - 1) * xscale + 2.0 * (xscale < 1.0 ? 1.0 : xscale) + 3.0) : tile;
    const size_t lds = (((size_t)span * C + 6) & ~(size_t)3) + (C == 3 ? (((size_t)span + 3) & ~(size_t)3) : 0);

    bool rec = prof && prof->begin(st);
    ingest_grey_rows_kernel<<<dim3(g.nrows, tiles, N), kThreads, lds, st>>>(img, (size_t)sh * row_stride_bytes, row_stride_bytes, C, wb, wg, wr,
                                                                            shift, g.r0, dx, W, tile, hpass ? xbounds_dev : nullptr,
                                                                            hpass ? xkk_dev : nullptr, xksize, tmp, g.nrows);
    if (rec) prof->end(st, PK_KERNEL_INGEST_GREY_ROWS, 0.0, (double)N * g.nrows * ((double)(hpass ? sw : W) * C + W));
    SN_LAUNCH_CHECK("ingest_grey_rows_kernel");

    rec = prof && prof->begin(st);
    ingest_grey_cols_kernel<<<dim3(cdiv(W, kThreads), H, N), kThreads, 0, st>>>(tmp, g.nrows, g.r0, dy, H, W, vpass ? ybounds_dev : nullptr,
                                                                                vpass ? ykk_dev : nullptr, yksize, lut256_dev, out);
    if (rec) prof->end(st, PK_KERNEL_INGEST_GREY_COLS, 0.0, (double)N * ((double)g.nrows * W + 4.0 * H * W));
    SN_LAUNCH_CHECK("ingest_grey_cols_kernel");
    return STABNET_OK;
}

int stabnet_ingest_colour(const unsigned char* img, int N, int sh, int sw, int C, size_t row_stride_bytes, int H, int W,
                          const int* xofs_dev, const short* xcoef_dev, const int* yofs_dev, const short* ycoef_dev, unsigned char* out,
                          void* stream, void* profp) {
    SN_REQUIRE(img && xofs_dev && xcoef_dev && yofs_dev && ycoef_dev && out, "ingest_colour: null pointer");
    SN_REQUIRE(C == 3, "ingest_colour: C must be 3 (BGR), got %d", C);
    SN_REQUIRE(N >= 1 && N <= 65535 && sh >= 1 && sw >= 1 && H >= 1 && W >= 1, "ingest_colour: batch (1..65535) and every size must be >= 1");
    SN_REQUIRE(row_stride_bytes >= (size_t)sw * C, "ingest_colour: row stride %zu < %d * %d bytes", row_stride_bytes, sw, C);
    const double xscale = (double)sw / (double)W;
    const int cap = 4096;                                                    // source pixels of one tile: two rows of 3 B = 24 KB of LDS
    const int tile = tile_of(W, xscale, 4.0, cap);
    const int tiles = cdiv(W, tile);
    SN_REQUIRE(tiles <= 65535, "ingest_colour: %d column tiles > 65535", tiles);
    hipStream_t st = (hipStream_t)stream;
    int rc = sn_check_device(img, "ingest_colour: img", st);
    if (rc == 0) rc = sn_check_device(out, "ingest_colour: out", st);
    if (rc) return rc;
    Prof* prof = static_cast<Prof*>(profp);
    const long span = (long)((tile - 1) * xscale + 4.0) < sw ? (long)((tile - 1) * xscale + 4.0) : sw;
    const size_t lds = 2 * (((size_t)span * C + 6) & ~(size_t)3);
    const bool rec = prof && prof->begin(st);
    ingest_colour_kernel<<<dim3(H, tiles, N), kThreads, lds, st>>>(img, (size_t)sh * row_stride_bytes, row_stride_bytes, C, H, W, tile, xofs_dev,
                                                                   xcoef_dev, yofs_dev, ycoef_dev, out);
    if (rec) prof->end(st, PK_KERNEL_INGEST_COLOUR, 0.0, (double)N * C * ((double)(sh < 2 * H ? sh : 2 * H) * sw + (double)H * W));
    SN_LAUNCH_CHECK("ingest_colour_kernel");
    return STABNET_OK;
}

}  // extern "C"
