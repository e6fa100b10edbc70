// Full-frame output (include/stabnet_hip.h, "full-frame output"; tests/mosaic_model.py is the executable statement), gfx950.
// A pixel the current stabilised frame does not cover is taken from what earlier stabilised frames showed there, moved by one
// homography between the two stabilised frames; inside a feather band at the frame's edge the two are blended.
//   mosaic_guard_kernel    : one workgroup per pair drops the matches that lie within `guard` pixels of an uncovered pixel (the
//                            content / black edge is the strongest corner of its cell and moves with the border, not the scene);
//                            ordered compaction through wave ballots and sixteen LDS slots, no atomics.
//   mosaic_compose_kernel  : one launch per frame over the output pixels.  Deeper than the feather band a pixel is the warped
//                            frame's, streamed (12 bytes in, 12 + 4 out per four pixels, the coordinates as two float4); in the band
//                            and outside the frame the previous canvas is gathered bilinearly at 1/32 px (integer weights, six
//                            contiguous bytes per row).  The homography and its status are read from device memory when the kernel runs.
// The remap's 1/32-px quantisation and its six-byte load are restated here; csrc/remap.hip is not touched (see its line 164).
#include <climits>
#include <cmath>
#include <cstdlib>
#include <initializer_list>

#include "common.h"

namespace {

constexpr int kGuardThreads = 1024, kWave = 64, kGuardWaves = kGuardThreads / kWave;     // a pair's rows in one chunk: a row per thread
constexpr int kMaxRows = 1024, kMaxGuard = 16, kEmpty = 255, kMaxRowsPerBlock = 8;

// ---- the guard ----
// one end of a row: X = ((xn + 1) * W) * 0.5, rounded to the nearest pixel; the (2 guard + 1)^2 box about it lies inside the image
// and every black in it is < 0.5.  (Every comparison is false for a NaN.)
__device__ __forceinline__ bool mosaic_end_safe(float xn, float yn, const float* __restrict__ black, int H, int W, int guard) {
    const float X = __fmul_rn(__fmul_rn(__fadd_rn(xn, 1.0f), (float)W), 0.5f), Y = __fmul_rn(__fmul_rn(__fadd_rn(yn, 1.0f), (float)H), 0.5f);
    const float xr = rintf(X), yr = rintf(Y), g = (float)guard;
    if (!(xr - g >= 0.0f && xr + g <= (float)(W - 1) && yr - g >= 0.0f && yr + g <= (float)(H - 1))) return false;
    const int xi = (int)xr, yi = (int)yr;                                      // guard .. W - 1 - guard: the box is inside
    for (int dy = -guard; dy <= guard; ++dy) {
        const float* row = black + (size_t)(yi + dy) * W + xi;
        bool bad = false;                                                      // one exit per box row: its loads do not wait for each other
        for (int dx = -guard; dx <= guard; ++dx) bad |= !(row[dx] < 0.5f);
        if (bad) return false;
    }
    return true;
}

__global__ __launch_bounds__(kGuardThreads) void mosaic_guard_kernel(const float4* __restrict__ rows, const int* __restrict__ nrows,
        const float* __restrict__ black0, const float* __restrict__ black1, int M, int H, int W, int guard, float4* __restrict__ out,
        int* __restrict__ out_n) {
    __shared__ int sCnt[kGuardWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, pair = blockIdx.x;
    int n = nrows[pair];
    n = n < 0 ? 0 : (n > M ? M : n);                                           // nothing past row n (or M) is read
    const float* b0 = black0 + (size_t)pair * H * W;
    const float* b1 = black1 + (size_t)pair * H * W;
    int base = 0;                                                              // rows kept so far (the same in every thread)
    for (int start = 0; start < n; start += kGuardThreads) {
        const int i = start + tid;
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        bool keep = false;
        if (i < n) {
            r = rows[(size_t)pair * M + i];
            keep = mosaic_end_safe(r.x, r.y, b0, H, W, guard) && mosaic_end_safe(r.z, r.w, b1, H, W, guard);
        }
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) sCnt[wave] = __popcll(bal);
        __syncthreads();
        int off = base, total = 0;
#pragma unroll
        for (int w = 0; w < kGuardWaves; ++w) {
            off += w < wave ? sCnt[w] : 0;
            total += sCnt[w];
        }
        if (keep) out[(size_t)pair * M + off + before] = r;
        base += total;
        __syncthreads();                                                       // sCnt is rewritten by the next chunk
    }
    for (int i = base + tid; i < M; i += kGuardThreads) out[(size_t)pair * M + i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (tid == 0) out_n[pair] = base;
}

// ---- the composite ----
struct MosaicArgs {
    int SH, SW, feather_log2, max_age, rows, wide;   // rows per workgroup; wide: counts is 8-byte aligned
    double ax, cx, ay, cy, sx, tx, sy, ty;           // x_n = ax j + cx, j = sx x_n + tx (likewise y): rounded once per operation by the host
    double w_min;                                    // the float32 argument, widened
};

// csrc/remap.hip's remap_src_load6, restated: bytes p .. p+5 in the low 48 bits, nothing outside [lo, hi) is read
__device__ __forceinline__ unsigned long long mosaic_load6(const unsigned char* __restrict__ p, const unsigned char* lo, const unsigned char* hi) {
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

// csrc/remap.hip's quantisation of a float32 coordinate to 1/32 px (remap_src_coord), restated
__device__ __forceinline__ int mosaic_quant32(float p) {
    const float q = fminf(fmaxf(__fmul_rn(p, 32.0f), -2.0e9f), 2.0e9f);
    return (q == q) ? (int)rintf(q) : -2000000000;
}

__device__ __forceinline__ int mosaic_quant64(double p) {
    const double q = fmin(fmax(__dmul_rn(p, 32.0), -2.0e9), 2.0e9);
    return (q == q) ? (int)rint(q) : -2000000000;
}

__device__ __forceinline__ int mosaic_depth(float px, float py, int SH, int SW) {
    const int qx = mosaic_quant32(px), qy = mosaic_quant32(py);
    return min(min(qx, 32 * (SW - 1) - qx), min(qy, 32 * (SH - 1) - qy));
}

// G = B (Hm A), float64; every product and sum one rounded operation, in the header's order
struct MosaicG { double g[9]; };
__device__ __forceinline__ MosaicG mosaic_pixel_homography(const float* __restrict__ Hm, const MosaicArgs& a) {
    double h[9], m[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = (double)Hm[k];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        m[3 * r + 0] = __dmul_rn(h[3 * r + 0], a.ax);
        m[3 * r + 1] = __dmul_rn(h[3 * r + 1], a.ay);
        m[3 * r + 2] = __dadd_rn(__dadd_rn(__dmul_rn(h[3 * r + 0], a.cx), __dmul_rn(h[3 * r + 1], a.cy)), h[3 * r + 2]);
    }
    MosaicG G;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        G.g[c] = __dadd_rn(__dmul_rn(a.sx, m[c]), __dmul_rn(a.tx, m[6 + c]));
        G.g[3 + c] = __dadd_rn(__dmul_rn(a.sy, m[3 + c]), __dmul_rn(a.ty, m[6 + c]));
        G.g[6 + c] = m[6 + c];
    }
    return G;
}

// The history sample of output pixel (i, j): -> available; hist = B | G << 8 | R << 16, hage = 1 + the oldest counting tap.
__device__ __forceinline__ bool mosaic_history(const MosaicG& G, const MosaicArgs& a, int i, int j, const unsigned char* __restrict__ canvas,
        const unsigned char* __restrict__ age, unsigned& hist, int& hage) {
    const int SH = a.SH, SW = a.SW;
    const double dj = (double)j, di = (double)i;
    const double u = __dadd_rn(__dadd_rn(__dmul_rn(G.g[0], dj), __dmul_rn(G.g[1], di)), G.g[2]);
    const double v = __dadd_rn(__dadd_rn(__dmul_rn(G.g[3], dj), __dmul_rn(G.g[4], di)), G.g[5]);
    const double w = __dadd_rn(__dadd_rn(__dmul_rn(G.g[6], dj), __dmul_rn(G.g[7], di)), G.g[8]);
    if (!(w > a.w_min)) return false;
    const int qx = mosaic_quant64(__ddiv_rn(u, w)), qy = mosaic_quant64(__ddiv_rn(v, w));
    const int ix = qx >> 5, iy = qy >> 5, fx = qx & 31, fy = qy & 31;
    // every tap with a nonzero weight lies inside the frame (tap [0][0] always has one)
    if (ix < 0 || iy < 0 || ix + (fx != 0 ? 1 : 0) > SW - 1 || iy + (fy != 0 ? 1 : 0) > SH - 1) return false;
    // The four ages and the two six-byte rows are loaded together, before anything is decided: one round trip to memory per sample
    // (with the ages checked first it was two, and a thread's samples follow each other).  A tap without weight is read where its
    // neighbour with weight lies (ox, oy = 0): inside the frame, and without effect on the oldest age or on the sum.
    const size_t p0 = (size_t)iy * SW + ix, ox = fx != 0 ? 1 : 0, oy = fy != 0 ? (size_t)SW : 0;
    const int a00 = age[p0], a01 = age[p0 + ox], a10 = age[p0 + oy], a11 = age[p0 + oy + ox];
    const unsigned char* end = canvas + (size_t)SH * SW * 3;
    const unsigned long long r0 = mosaic_load6(canvas + p0 * 3, canvas, end);
    const unsigned long long r1 = mosaic_load6(canvas + (p0 + oy) * 3, canvas, end);
    const int amax = max(max(a00, a01), max(a10, a11));
    const int w00 = (32 - fy) * (32 - fx), w01 = (32 - fy) * fx, w10 = fy * (32 - fx), w11 = fy * fx;         // sum 1024
    hist = 0u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int acc = (int)((r0 >> (8 * ch)) & 0xff) * w00 + (int)((r0 >> (24 + 8 * ch)) & 0xff) * w01 +
                        (int)((r1 >> (8 * ch)) & 0xff) * w10 + (int)((r1 >> (24 + 8 * ch)) & 0xff) * w11;
        hist |= (unsigned)((acc + 512) >> 10) << (8 * ch);
    }
    hage = amax + 1;
    return amax < kEmpty && amax + 1 <= a.max_age;
}

// One pixel outside the pure-fresh case (d < F): the combine table.  -> colour (24 bits), age; cls 1 blended, 2 history, 3 empty, 0 fresh
__device__ __forceinline__ unsigned mosaic_band_pixel(const MosaicG& G, bool model, const MosaicArgs& a, int i, int j, int d, unsigned warped,
        const unsigned char* __restrict__ canvas, const unsigned char* __restrict__ age, int& out_age, int& cls) {
    unsigned hist = 0u;
    int hage = 0;
    const bool avail = model && mosaic_history(G, a, i, j, canvas, age, hist, hage);
    const bool covered = d >= 0;
    if (!avail) {
        out_age = covered ? 0 : kEmpty;
        cls = covered ? 0 : 3;
        return covered ? warped : 0u;
    }
    if (!covered) { out_age = hage; cls = 2; return hist; }
    const int Fq = 32 << a.feather_log2, wa = min(max(d, 0), Fq);
    unsigned o = 0u;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int b = ((int)((warped >> (8 * ch)) & 0xff) * wa + (int)((hist >> (8 * ch)) & 0xff) * (Fq - wa) + (Fq >> 1)) >> (5 + a.feather_log2);
        o |= (unsigned)b << (8 * ch);
    }
    out_age = 2 * wa >= Fq ? 0 : hage;
    cls = 1;
    return o;
}

// The workgroup's class counts: two words per thread (blended | history << 16, and empty; at most 512 * 4 * kMaxRowsPerBlock pixels a
// workgroup), summed over the wave by shuffles, over the waves through LDS; thread 0 adds the nonzero ones to counts[n] (integer
// sums: any order).  All adds of a frame go to one 16-byte record, and adds to one address are served one after the other at the
// memory side (about 90 per microsecond): with one row segment per workgroup and four adds each, a 720p frame waited 50 us for its
// 4,300 adds.  So a workgroup covers several rows, and with counts 8-byte aligned (wide) its four sums leave as two 64-bit adds of two
// counters each (no carry crosses the halves: a frame's sums stay below 2^31; the caller zeroes counts per frame).
__device__ __forceinline__ void mosaic_count(unsigned packed, unsigned empty, unsigned pixels, int* __restrict__ counts, bool wide) {
    __shared__ unsigned sPk[8], sEm[8];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        packed += __shfl_xor(packed, off);
        empty += __shfl_xor(empty, off);
    }
    const int wave = threadIdx.x >> 6, waves = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) { sPk[wave] = packed; sEm[wave] = empty; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < waves; ++k) { packed += sPk[k]; empty += sEm[k]; }
    const unsigned blended = packed & 0xffffu, hist = packed >> 16, fresh = pixels - blended - hist - empty;
    if (wide) {
        unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
        if (fresh | blended) atomicAdd(c, (unsigned long long)fresh | ((unsigned long long)blended << 32));
        if (hist | empty) atomicAdd(c + 1, (unsigned long long)hist | ((unsigned long long)empty << 32));
        return;
    }
    if (fresh) atomicAdd(counts + 0, (int)fresh);
    if (blended) atomicAdd(counts + 1, (int)blended);
    if (hist) atomicAdd(counts + 2, (int)hist);
    if (empty) atomicAdd(counts + 3, (int)empty);
}

// What a thread reads of one row: PX consecutive pixels from `pix` on.  PX == 4 (SW % 4 == 0, warped 4-byte and px, py 16-byte
// aligned): three dwords and two float4; PX == 1: three bytes (packed into w[0]) and two floats, any width and alignment.
template <int PX> struct MosaicIn { unsigned w[PX == 4 ? 3 : 1]; float x[PX], y[PX]; };

template <int PX>
__device__ __forceinline__ MosaicIn<PX> mosaic_load(const unsigned char* __restrict__ warped, const float* __restrict__ px,
                                                    const float* __restrict__ py, size_t pix) {
    MosaicIn<PX> in;
    if constexpr (PX == 4) {
        const unsigned* wp = reinterpret_cast<const unsigned*>(warped + pix * 3);
        in.w[0] = wp[0]; in.w[1] = wp[1]; in.w[2] = wp[2];
        const float4 x4 = *reinterpret_cast<const float4*>(px + pix), y4 = *reinterpret_cast<const float4*>(py + pix);
        in.x[0] = x4.x; in.x[1] = x4.y; in.x[2] = x4.z; in.x[3] = x4.w;
        in.y[0] = y4.x; in.y[1] = y4.y; in.y[2] = y4.z; in.y[3] = y4.w;
    } else {
        in.w[0] = (unsigned)warped[pix * 3] | ((unsigned)warped[pix * 3 + 1] << 8) | ((unsigned)warped[pix * 3 + 2] << 16);
        in.x[0] = px[pix]; in.y[0] = py[pix];
    }
    return in;
}

// grid (cdiv(SW / PX, blockDim.x), cdiv(SH, a.rows), N): a workgroup covers a segment of a.rows consecutive rows, a thread PX
// consecutive pixels of each; the next row's loads are issued before the current row is worked on.  Deeper than the band a pixel
// streams through; the homography is built once per thread, when its first band pixel asks for it.
template <int PX>
__global__ __launch_bounds__(512) void mosaic_compose_kernel(const unsigned char* __restrict__ warped, const float* __restrict__ px,
        const float* __restrict__ py, const unsigned char* __restrict__ canvas_prev, const unsigned char* __restrict__ age_prev,
        const float* __restrict__ Hm, const int* __restrict__ status, MosaicArgs a, unsigned char* __restrict__ canvas_cur,
        unsigned char* __restrict__ age_cur, int* __restrict__ counts) {
    const int j0 = (blockIdx.x * blockDim.x + threadIdx.x) * PX, n = blockIdx.z;
    const int i0 = blockIdx.y * a.rows, i1 = min(i0 + a.rows, a.SH);
    const size_t frame = (size_t)n * a.SH * a.SW;
    const int Fq = 32 << a.feather_log2;
    unsigned packed = 0u, empty = 0u;
    if (j0 < a.SW) {
        bool ready = false, model = false;
        MosaicG G = {};
        MosaicIn<PX> cur = mosaic_load<PX>(warped, px, py, frame + (size_t)i0 * a.SW + j0);
        for (int i = i0; i < i1; ++i) {
            const size_t pix = frame + (size_t)i * a.SW + j0;
            MosaicIn<PX> nxt = cur;
            if (i + 1 < i1) nxt = mosaic_load<PX>(warped, px, py, pix + a.SW);
            int d[PX], dmin = INT_MAX;
#pragma unroll
            for (int e = 0; e < PX; ++e) {
                d[e] = mosaic_depth(cur.x[e], cur.y[e], a.SH, a.SW);
                dmin = min(dmin, d[e]);
            }
            unsigned ages = 0u;
            if (dmin < Fq) {                                                    // the band: the frame's edge only
                if (!ready) {
                    const int st = status[n];
                    model = st == 1 || st == 2;
                    if (model) G = mosaic_pixel_homography(Hm + 9 * (size_t)n, a);
                    ready = true;
                }
                unsigned in[PX], o[PX];
                if constexpr (PX == 4) {
                    in[0] = cur.w[0] & 0xffffffu;
                    in[1] = (unsigned)(((((unsigned long long)cur.w[1]) << 32) | cur.w[0]) >> 24) & 0xffffffu;
                    in[2] = (unsigned)(((((unsigned long long)cur.w[2]) << 32) | cur.w[1]) >> 16) & 0xffffffu;
                    in[3] = cur.w[2] >> 8;
                } else {
                    in[0] = cur.w[0];
                }
#pragma unroll
                for (int e = 0; e < PX; ++e) {
                    o[e] = in[e];
                    if (d[e] < Fq) {
                        int oa, cls;
                        o[e] = mosaic_band_pixel(G, model, a, i, j0 + e, d[e], in[e], canvas_prev + frame * 3, age_prev + frame, oa, cls);
                        ages |= (unsigned)oa << (8 * e);
                        packed += cls == 1 ? 1u : (cls == 2 ? 1u << 16 : 0u);
                        empty += cls == 3 ? 1u : 0u;
                    }
                }
                if constexpr (PX == 4) {
                    cur.w[0] = o[0] | (o[1] << 24);
                    cur.w[1] = (o[1] >> 8) | (o[2] << 16);
                    cur.w[2] = (o[2] >> 16) | (o[3] << 8);
                } else {
                    cur.w[0] = o[0];
                }
            }
            if constexpr (PX == 4) {
                unsigned* op = reinterpret_cast<unsigned*>(canvas_cur + pix * 3);
                op[0] = cur.w[0]; op[1] = cur.w[1]; op[2] = cur.w[2];
                *reinterpret_cast<unsigned*>(age_cur + pix) = ages;
            } else {
                canvas_cur[pix * 3] = (unsigned char)(cur.w[0] & 0xff);
                canvas_cur[pix * 3 + 1] = (unsigned char)((cur.w[0] >> 8) & 0xff);
                canvas_cur[pix * 3 + 2] = (unsigned char)((cur.w[0] >> 16) & 0xff);
                age_cur[pix] = (unsigned char)ages;
            }
            cur = nxt;
        }
    }
    const unsigned width = (unsigned)min(a.SW - (int)(blockIdx.x * blockDim.x) * PX, (int)blockDim.x * PX);
    mosaic_count(packed, empty, width * (unsigned)(i1 - i0), counts + 4 * (size_t)n, a.wide != 0);
}

// STABNET_MOSAIC_ROWS=1..8: rows per workgroup of the composing kernels (debug switch for A/B runs; read once).  Default 2, measured
// (DESIGN.md Round 17): one row leaves twice the adds on the counters' one address, four rows put four band rows behind each other.
static int mosaic_rows_per_block() {
    static const int rows = []() { const char* v = getenv("STABNET_MOSAIC_ROWS"); const int r = v ? atoi(v) : 2; return r < 1 ? 1 : (r > kMaxRowsPerBlock ? kMaxRowsPerBlock : r); }();
    return rows;
}

}  // namespace

extern "C" {

/* See include/stabnet_hip.h. */
int stabnet_mosaic_guard_matches(const float* matches, const int* n, const float* black0, const float* black1, int B, int M, int H, int W,
                                 int guard, float* out_matches, int* out_n, void* stream) {
    SN_REQUIRE(matches && n && black0 && black1 && out_matches && out_n, "mosaic_guard_matches: null pointer");
    SN_REQUIRE(out_matches != matches, "mosaic_guard_matches: out_matches must not be matches (the compaction is not in place)");
    SN_REQUIRE(B >= 1 && B <= 65535, "mosaic_guard_matches: B must be 1..65535, got %d", B);
    SN_REQUIRE(M >= 4 && M <= kMaxRows, "mosaic_guard_matches: M must be 4..%d, got %d", kMaxRows, M);
    SN_REQUIRE(guard >= 0 && guard <= kMaxGuard, "mosaic_guard_matches: guard must be 0..%d pixels, got %d", kMaxGuard, guard);
    SN_REQUIRE(H >= 1 && H <= 1 << 20 && W >= 1 && W <= 1 << 20, "mosaic_guard_matches: H and W must be 1..2^20, got %d x %d", H, W);
    SN_REQUIRE((((uintptr_t)matches | (uintptr_t)out_matches) & 15) == 0, "mosaic_guard_matches: matches and out_matches must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    for (const void* p : {(const void*)matches, (const void*)n, (const void*)black0, (const void*)black1, (const void*)out_matches,
                          (const void*)out_n}) {
        const int rc = sn_check_device(p, "mosaic_guard_matches: a pointer", st);
        if (rc) return rc;
    }
    mosaic_guard_kernel<<<dim3(B), kGuardThreads, 0, st>>>(reinterpret_cast<const float4*>(matches), n, black0, black1, M, H, W, guard,
                                                           reinterpret_cast<float4*>(out_matches), out_n);
    SN_LAUNCH_CHECK("mosaic_guard_kernel");
    return STABNET_OK;
}

/* See include/stabnet_hip.h. */
int stabnet_mosaic_compose(const unsigned char* warped, const float* px, const float* py, const unsigned char* canvas_prev,
                           const unsigned char* age_prev, const float* Hm, const int* status, int N, int SH, int SW, int H, int W,
                           int feather_log2, int max_age, float w_min, unsigned char* canvas_cur, unsigned char* age_cur, int* counts,
                           void* stream) {
    SN_REQUIRE(warped && px && py && canvas_prev && age_prev && Hm && status && canvas_cur && age_cur && counts, "mosaic_compose: null pointer");
    SN_REQUIRE(N >= 1 && N <= 65535, "mosaic_compose: batch %d outside 1..65535", N);
    SN_REQUIRE(SH >= 1 && SH <= 32767 && SW >= 1 && SW <= 32767, "mosaic_compose: frame %dx%d outside 1..32767", SH, SW);
    SN_REQUIRE(H >= 1 && H <= 1 << 20 && W >= 1 && W <= 1 << 20, "mosaic_compose: H and W must be 1..2^20, got %d x %d", H, W);
    SN_REQUIRE(feather_log2 >= 0 && feather_log2 <= 6, "mosaic_compose: feather_log2 must be 0..6 (1..64 px), got %d", feather_log2);
    SN_REQUIRE(max_age >= 1 && max_age <= 254, "mosaic_compose: max_age must be 1..254, got %d", max_age);
    SN_REQUIRE(w_min >= 0.0f && w_min < INFINITY, "mosaic_compose: w_min must be finite and not negative, got %g", w_min);
    SN_REQUIRE(canvas_cur != canvas_prev && age_cur != age_prev, "mosaic_compose: the current canvas and ages must not be the previous ones");
    hipStream_t st = (hipStream_t)stream;
    for (const void* p : {(const void*)warped, (const void*)px, (const void*)py, (const void*)canvas_prev, (const void*)age_prev, (const void*)Hm,
                          (const void*)status, (const void*)canvas_cur, (const void*)age_cur, (const void*)counts}) {
        const int rc = sn_check_device(p, "mosaic_compose: a pointer", st);
        if (rc) return rc;
    }
    MosaicArgs a;
    a.SH = SH; a.SW = SW; a.feather_log2 = feather_log2; a.max_age = max_age;
    a.ax = 2.0 / SW; a.cx = (1.0 / SW - 1.0 / W) - 1.0;
    a.ay = 2.0 / SH; a.cy = (1.0 / SH - 1.0 / H) - 1.0;
    a.sx = 0.5 * SW; a.tx = (0.5 * SW + (0.5 * SW) / W) - 0.5;
    a.sy = 0.5 * SH; a.ty = (0.5 * SH + (0.5 * SH) / H) - 0.5;
    a.w_min = (double)w_min;
    const bool v4 = SW % 4 == 0 && (((uintptr_t)warped | (uintptr_t)canvas_cur | (uintptr_t)age_cur) & 3) == 0 &&
                    (((uintptr_t)px | (uintptr_t)py) & 15) == 0;
    a.rows = mosaic_rows_per_block();
    a.wide = ((uintptr_t)counts & 7) == 0;
    const int items = v4 ? SW / 4 : SW, threads = items >= 512 ? 512 : ((items + 63) & ~63);      // whole waves, a segment of a.rows rows each
    const dim3 grid(cdiv(items, threads), cdiv(SH, a.rows), N);
    if (v4) mosaic_compose_kernel<4><<<grid, threads, 0, st>>>(warped, px, py, canvas_prev, age_prev, Hm, status, a, canvas_cur, age_cur, counts);
    else mosaic_compose_kernel<1><<<grid, threads, 0, st>>>(warped, px, py, canvas_prev, age_prev, Hm, status, a, canvas_cur, age_cur, counts);
    SN_LAUNCH_CHECK(v4 ? "mosaic_compose_kernel<4>" : "mosaic_compose_kernel<1>");
    return STABNET_OK;
}

}  // extern "C"
