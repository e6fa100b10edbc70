// Batched TV-L1 optical flow (Zach / Pock / Bischof in the IPOL formulation of Sanchez, Meinhardt-Llopis, Facciolo), cut down so
// that every step is a deterministic float32 stencil: a fixed number of inner iterations (no epsilon stop: its global sum would
// make the iteration count depend on the summation order), no median filter, bilinear warps, a pyramid factor of exactly 2.
// tests/tvl1_model.py is the same arithmetic in NumPy and the yardstick: every operation below is one explicitly rounded float32
// operation (__fadd_rn, __fmul_rn, __fdiv_rn, sqrtf), in the model's order, and the library is built with -ffp-contract=off.
//
//   pyramid   down = [1,4,6,4,1]/16 along x, then along y, replicated borders, then the pixels at even (y, x): ceil(n/2)
//   level     u = 2 * upsample(u of the coarser level) (half-pixel centred bilinear) or 0; p11 p12 p21 p22 = 0; I1x, I1y centred
//   warp      Ix, Iy, Iw = I1x, I1y, I1 at (x + u1, y + u2), clamped; g = Ix*Ix + Iy*Iy; rc = ((Iw - Ix*u1) - Iy*u2) - I0
//   iteration rho = (rc + Ix*u1) + Iy*u2; f = lt | -lt | -rho/g | 0; u = (u + f*(Ix, Iy)) + theta*div(p);
//             p = (p + taut*grad(u)) / (1 + taut*|grad(u)|)            (lt = lambda*theta, taut = tau/theta, both float32)
//
// The iteration is the hot path: hundreds of dependent sweeps over ten floats per pixel.  tvl1_step_kernel is one sweep per launch
// (the plain path and the A/B leg); tvl1_fused_kernel runs up to kK sweeps per launch by temporal blocking: a workgroup owns a
// kTX x kTY tile, loads it with a halo of kK pixels, keeps every pixel's state and constants in REGISTERS (a thread owns kPPT
// pixels of the region) and exchanges only what a neighbour reads -- u1, u2 and the four duals -- through LDS.  A sweep reads the
// duals of the left / upper neighbour and the new u of the right / lower one, so whatever is wrong at the rim of the region moves
// inwards by one pixel per sweep and never reaches the tile in kK sweeps; the image's own border rules read nothing outside the
// image, so pixels outside it are never computed and never read.  Both kernels call the same two device functions per pixel, so
// every pixel sees the same operations in the same order and the two paths write the same bits.
// State planes [6][B][H][W] = u1, u2, p11, p12, p21, p22; constants [4][B][H][W] = Ix, Iy, rc, g.  A sweep cannot run in place
// (a neighbouring workgroup still reads the old values), so the launches alternate between two state buffers.
// No atomics, no allocation, no host copy, nothing read back: the whole solve sits on one stream and can be captured in a graph.
#include <cmath>
#include <cstdlib>
#include <initializer_list>
#include <cstring>

#include "common.h"
#include "prof.h"
#include "tvl1_shared.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxLevels = 16;
constexpr int kSX = 64, kSY = 4;                           // stepwise tile: kSX * kSY = kThreads, u on the tile + one ring right / below

// fused: kK sweeps per launch on a kTX x kTY tile.  The region (tile + halo) is 64 x 64 = 4096 pixels, four per thread of a 1024-thread
// workgroup (a wave owns one row of the region at a time): 40 floats of state and constants per thread in registers, 6 planes of
// LDS, one workgroup (16 waves) per CU.  Every plane has kPad floats in front and behind, so that the neighbour reads of the
// region's rim (l - 1, l - kRW, l + 1, l + kRW) stay inside it without a guard; what they return there is never used.
constexpr int kK = 5, kRW = 64, kRH = 64, kRN = kRW * kRH, kTX = kRW - 2 * kK, kTY = kRH - 2 * kK, kFThreads = 1024;
constexpr int kPPT = kRN / kFThreads, kPad = kRW, kPlane = kRN + 2 * kPad;                  // 6 planes = 101376 B
static_assert(kSX * kSY == kThreads, "stepwise tile");
static_assert(kPPT * kFThreads == kRN && kPad >= kRW && 6 * kPlane * 4 <= 160 * 1024, "fused region");

enum : unsigned { F_IN = 1, F_X0 = 2, F_XL = 4, F_Y0 = 8, F_YL = 16, F_STORE = 32 };

// ---- per-pixel arithmetic shared by the stepwise and the fused kernel -----------------------------------------------------------------

// one axis of the backward-difference divergence: p itself in the first column / row, -p[x-1] in the last, p[x] - p[x-1] between
// (both candidates are computed first, so that the choice is a select and not a branch around a subtraction)
__device__ __forceinline__ float tv_div1(float p, float prev, bool first, bool last) {
    const float d = __fsub_rn(p, prev), n = -prev, r = last ? n : d;
    return first ? p : r;
}

__device__ __forceinline__ void tv_u_update(float& u1, float& u2, float ix, float iy, float rc, float g, float d1, float d2, float lt,
                                            float theta) {
    const float rho = __fadd_rn(__fadd_rn(rc, __fmul_rn(ix, u1)), __fmul_rn(iy, u2));
    const float lg = __fmul_rn(lt, g);
    const float q = __fdiv_rn(-rho, g);                                             // selects, not branches: the first rule that holds wins
    float f = g > 1e-10f ? q : 0.0f;
    f = rho > lg ? -lt : f;
    f = rho < -lg ? lt : f;
    u1 = __fadd_rn(__fadd_rn(u1, __fmul_rn(f, ix)), __fmul_rn(theta, d1));
    u2 = __fadd_rn(__fadd_rn(u2, __fmul_rn(f, iy)), __fmul_rn(theta, d2));
}

// (sqrtf, not __fsqrt_rn: this compiler's __fsqrt_rn is the native approximate instruction; sqrtf is correctly rounded by default)
// the two duals of one flow component: forward differences of the new u (zero in the last column / row)
__device__ __forceinline__ void tv_p_update(float& pa, float& pb, float u, float right, float down, bool lastx, bool lasty, float taut) {
    const float da = __fsub_rn(right, u), db = __fsub_rn(down, u), a = lastx ? 0.0f : da, b = lasty ? 0.0f : db;
    const float n = __fadd_rn(1.0f, __fmul_rn(taut, sqrtf(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)))));
    pa = __fdiv_rn(__fadd_rn(pa, __fmul_rn(taut, a)), n);
    pb = __fdiv_rn(__fadd_rn(pb, __fmul_rn(taut, b)), n);
}

// ---- stage kernels: grid (cdiv(h * w, kThreads), B), one thread per output pixel, indexed by absolute position ------------------------

__global__ __launch_bounds__(kThreads) void tvl1_down_kernel(const float* __restrict__ in, int ps, TvAff af, int H, int W,
                                                             float* __restrict__ out, int h, int w) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= h * w) return;
    const int yo = p / w, xo = p - yo * w, cy = 2 * yo, cx = 2 * xo;
    const float k[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const float* img = in + (size_t)blockIdx.y * H * W * ps;
    int xs[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int x = cx - 2 + i;
        xs[i] = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
    }
    float acc = 0.0f;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        int y = cy - 2 + r;
        y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
        const float* row = img + (size_t)y * W * ps;
        float t = __fmul_rn(k[0], tv_px(row[(size_t)xs[0] * ps], af));
#pragma unroll
        for (int i = 1; i < 5; ++i) t = __fadd_rn(t, __fmul_rn(k[i], tv_px(row[(size_t)xs[i] * ps], af)));
        acc = r == 0 ? __fmul_rn(k[0], t) : __fadd_rn(acc, __fmul_rn(k[r], t));
    }
    out[(size_t)blockIdx.y * h * w + p] = acc;
}

__global__ __launch_bounds__(kThreads) void tvl1_grad_kernel(const float* __restrict__ in, int ps, TvAff af, int H, int W,
                                                             float* __restrict__ gx, float* __restrict__ gy) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= H * W) return;
    const int y = p / W, x = p - y * W;
    const float* img = in + (size_t)blockIdx.y * H * W * ps;
    const int xm = x > 0 ? x - 1 : 0, xp = x < W - 1 ? x + 1 : W - 1, ym = y > 0 ? y - 1 : 0, yp = y < H - 1 ? y + 1 : H - 1;
    const size_t o = (size_t)blockIdx.y * H * W + p;
    gx[o] = __fmul_rn(0.5f, __fsub_rn(tv_px(img[((size_t)y * W + xp) * ps], af), tv_px(img[((size_t)y * W + xm) * ps], af)));
    gy[o] = __fmul_rn(0.5f, __fsub_rn(tv_px(img[((size_t)yp * W + x) * ps], af), tv_px(img[((size_t)ym * W + x) * ps], af)));
}

// u: [2][B][H][W]; cst: [4][B][H][W] = Ix, Iy, rc, g; n = B * H * W
__global__ __launch_bounds__(kThreads) void tvl1_warp_kernel(const float* __restrict__ i0, const float* __restrict__ i1, int ps, TvAff af,
                                                             const float* __restrict__ gx, const float* __restrict__ gy,
                                                             const float* __restrict__ u, float* __restrict__ cst, size_t n, int H, int W) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= H * W) return;
    const int y = p / W, x = p - y * W;
    const size_t hw = (size_t)H * W, o = blockIdx.y * hw + p;
    const float u1 = u[o], u2 = u[n + o];
    const float xs = __fadd_rn((float)x, u1), ys = __fadd_rn((float)y, u2);
    const TvAff none = {0.0f, 1.0f, 0};
    const float iw = tv_bilinear(i1 + blockIdx.y * hw * ps, ps, H, W, ys, xs, af);
    const float ix = tv_bilinear(gx + blockIdx.y * hw, 1, H, W, ys, xs, none);
    const float iy = tv_bilinear(gy + blockIdx.y * hw, 1, H, W, ys, xs, none);
    cst[o] = ix;
    cst[n + o] = iy;
    cst[2 * n + o] = __fsub_rn(__fsub_rn(__fsub_rn(iw, __fmul_rn(ix, u1)), __fmul_rn(iy, u2)), tv_px(i0[o * ps], af));
    cst[3 * n + o] = __fadd_rn(__fmul_rn(ix, ix), __fmul_rn(iy, iy));
}

// grid.z = plane (u1, u2): in [2][B][h][w] -> out [2][B][H][W]
__global__ __launch_bounds__(kThreads) void tvl1_up_kernel(const float* __restrict__ in, int h, int w, float* __restrict__ out, int H, int W,
                                                           int B) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= H * W) return;
    const int y = p / W, x = p - y * W;
    const size_t img = (size_t)blockIdx.z * B + blockIdx.y;
    const float sy = __fsub_rn(__fmul_rn(__fadd_rn((float)y, 0.5f), 0.5f), 0.5f), sx = __fsub_rn(__fmul_rn(__fadd_rn((float)x, 0.5f), 0.5f), 0.5f);
    out[img * H * W + p] = __fmul_rn(2.0f, tv_bilinear(in + img * h * w, 1, h, w, sy, sx, TvAff{0.0f, 1.0f, 0}));
}

// u [2][B][H][W] -> uv [B][H][W][2] (pixels) and / or map [B][H][W][2] (what interpolate() reads: xp = (x + 1) * W / 2)
__global__ __launch_bounds__(kThreads) void tvl1_map_kernel(const float* __restrict__ u, size_t n, float* __restrict__ uv,
                                                            float* __restrict__ map, int H, int W) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= H * W) return;
    const int y = p / W, x = p - y * W;
    const size_t o = (size_t)blockIdx.y * H * W + p;
    const float u1 = u[o], u2 = u[n + o];
    if (uv) *reinterpret_cast<float2*>(uv + 2 * o) = make_float2(u1, u2);
    if (map)
        *reinterpret_cast<float2*>(map + 2 * o) =
            make_float2(__fsub_rn(__fdiv_rn(__fmul_rn(2.0f, __fadd_rn((float)x, u1)), (float)W), 1.0f),
                        __fsub_rn(__fdiv_rn(__fmul_rn(2.0f, __fadd_rn((float)y, u2)), (float)H), 1.0f));
}

// ---- one sweep per launch: grid (cdiv(W, kSX), cdiv(H, kSY), B) -----------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void tvl1_step_kernel(const float* __restrict__ sin, float* __restrict__ sout,
                                                             const float* __restrict__ cst, size_t n, int H, int W, float lt, float taut,
                                                             float theta) {
    __shared__ float s1[(kSY + 1) * (kSX + 1)], s2[(kSY + 1) * (kSX + 1)];
    const int x0 = blockIdx.x * kSX, y0 = blockIdx.y * kSY;
    const size_t img = (size_t)blockIdx.z * H * W;
    // the new u on the tile and one ring to the right and below (what the duals' forward differences read)
    for (int l = threadIdx.x; l < (kSY + 1) * (kSX + 1); l += kThreads) {
        const int ry = l / (kSX + 1), rx = l - ry * (kSX + 1), x = x0 + rx, y = y0 + ry;
        if (x >= W || y >= H) continue;
        const size_t o = img + (size_t)y * W + x;
        float u1 = sin[o], u2 = sin[n + o];
        const float p11 = sin[2 * n + o], p12 = sin[3 * n + o], p21 = sin[4 * n + o], p22 = sin[5 * n + o];
        const float l11 = x > 0 ? sin[2 * n + o - 1] : 0.0f, l21 = x > 0 ? sin[4 * n + o - 1] : 0.0f;
        const float t12 = y > 0 ? sin[3 * n + o - W] : 0.0f, t22 = y > 0 ? sin[5 * n + o - W] : 0.0f;
        const float d1 = __fadd_rn(tv_div1(p11, l11, x == 0, x == W - 1), tv_div1(p12, t12, y == 0, y == H - 1));
        const float d2 = __fadd_rn(tv_div1(p21, l21, x == 0, x == W - 1), tv_div1(p22, t22, y == 0, y == H - 1));
        tv_u_update(u1, u2, cst[o], cst[n + o], cst[2 * n + o], cst[3 * n + o], d1, d2, lt, theta);
        s1[l] = u1;
        s2[l] = u2;
    }
    __syncthreads();
    const int tx = threadIdx.x % kSX, ty = threadIdx.x / kSX, x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    const int l = ty * (kSX + 1) + tx;
    const size_t o = img + (size_t)y * W + x;
    const bool lastx = x == W - 1, lasty = y == H - 1;
    const float u1 = s1[l], u2 = s2[l];
    float p11 = sin[2 * n + o], p12 = sin[3 * n + o], p21 = sin[4 * n + o], p22 = sin[5 * n + o];
    tv_p_update(p11, p12, u1, lastx ? 0.0f : s1[l + 1], lasty ? 0.0f : s1[l + kSX + 1], lastx, lasty, taut);
    tv_p_update(p21, p22, u2, lastx ? 0.0f : s2[l + 1], lasty ? 0.0f : s2[l + kSX + 1], lastx, lasty, taut);
    sout[o] = u1;
    sout[n + o] = u2;
    sout[2 * n + o] = p11;
    sout[3 * n + o] = p12;
    sout[4 * n + o] = p21;
    sout[5 * n + o] = p22;
}

// ---- k <= kK sweeps per launch: grid (cdiv(W, kTX), cdiv(H, kTY), B) ------------------------------------------------------------------

__global__ __launch_bounds__(kFThreads) void tvl1_fused_kernel(const float* __restrict__ sin, float* __restrict__ sout,
                                                                  const float* __restrict__ cst, size_t n, int H, int W, float lt,
                                                                  float taut, float theta, int k) {
    __shared__ float sm[6][kPlane];                                                 // u1, u2, p11, p12, p21, p22 of the region
#define S(p, i) sm[p][kPad + (i)]
    const int gx0 = blockIdx.x * kTX - kK, gy0 = blockIdx.y * kTY - kK;
    const size_t img = (size_t)blockIdx.z * H * W;
    float u1[kPPT], u2[kPPT], p11[kPPT], p12[kPPT], p21[kPPT], p22[kPPT], ix[kPPT], iy[kPPT], rc[kPPT], g[kPPT];
    unsigned fl[kPPT];
#pragma unroll
    for (int j = 0; j < kPPT; ++j) {
        const int l = threadIdx.x + j * kFThreads, ry = l / kRW, rx = l - ry * kRW, x = gx0 + rx, y = gy0 + ry;
        const bool in = x >= 0 && x < W && y >= 0 && y < H;               // pixels outside the image are never computed
        unsigned f = 0;
        if (in) {
            f = F_IN | (x == 0 ? F_X0 : 0) | (x == W - 1 ? F_XL : 0) | (y == 0 ? F_Y0 : 0) | (y == H - 1 ? F_YL : 0) |
                (rx >= kK && rx < kK + kTX && ry >= kK && ry < kK + kTY ? F_STORE : 0);
            const size_t o = img + (size_t)y * W + x;
            u1[j] = sin[o]; u2[j] = sin[n + o]; p11[j] = sin[2 * n + o]; p12[j] = sin[3 * n + o]; p21[j] = sin[4 * n + o]; p22[j] = sin[5 * n + o];
            ix[j] = cst[o]; iy[j] = cst[n + o]; rc[j] = cst[2 * n + o]; g[j] = cst[3 * n + o];
        } else {
            u1[j] = u2[j] = p11[j] = p12[j] = p21[j] = p22[j] = ix[j] = iy[j] = rc[j] = g[j] = 0.0f;
        }
        fl[j] = f;
        S(2, l) = p11[j]; S(3, l) = p12[j]; S(4, l) = p21[j]; S(5, l) = p22[j];
    }
    __syncthreads();
    for (int it = 0; it < k; ++it) {
        // u: reads the duals of the left and the upper pixel.  At the rim of the region that neighbour was not loaded: the value
        // is wrong there, and the wrong ring grows inwards by one pixel per sweep -- kK of them never reach the tile.
#pragma unroll
        for (int j = 0; j < kPPT; ++j) {
            const int l = threadIdx.x + j * kFThreads;
            const unsigned f = fl[j];
            if (!(f & F_IN)) continue;
            const float l11 = S(2, l - 1), l21 = S(4, l - 1), t12 = S(3, l - kRW), t22 = S(5, l - kRW);
            const float d1 = __fadd_rn(tv_div1(p11[j], l11, f & F_X0, f & F_XL), tv_div1(p12[j], t12, f & F_Y0, f & F_YL));
            const float d2 = __fadd_rn(tv_div1(p21[j], l21, f & F_X0, f & F_XL), tv_div1(p22[j], t22, f & F_Y0, f & F_YL));
            tv_u_update(u1[j], u2[j], ix[j], iy[j], rc[j], g[j], d1, d2, lt, theta);
            S(0, l) = u1[j];
            S(1, l) = u2[j];
        }
        __syncthreads();
        // p: reads the new u of the right and the lower pixel
#pragma unroll
        for (int j = 0; j < kPPT; ++j) {
            const int l = threadIdx.x + j * kFThreads;
            const unsigned f = fl[j];
            if (!(f & F_IN)) continue;
            const bool lastx = f & F_XL, lasty = f & F_YL;
            const float r1 = S(0, l + 1), r2 = S(1, l + 1), b1 = S(0, l + kRW), b2 = S(1, l + kRW);
            tv_p_update(p11[j], p12[j], u1[j], r1, b1, lastx, lasty, taut);
            tv_p_update(p21[j], p22[j], u2[j], r2, b2, lastx, lasty, taut);
            S(2, l) = p11[j]; S(3, l) = p12[j]; S(4, l) = p21[j]; S(5, l) = p22[j];
        }
        __syncthreads();
    }
#undef S
#pragma unroll
    for (int j = 0; j < kPPT; ++j) {
        if (!(fl[j] & F_STORE)) continue;
        const int l = threadIdx.x + j * kFThreads, ry = l / kRW, rx = l - ry * kRW;
        const size_t o = img + (size_t)(gy0 + ry) * W + (gx0 + rx);
        sout[o] = u1[j]; sout[n + o] = u2[j]; sout[2 * n + o] = p11[j]; sout[3 * n + o] = p12[j]; sout[4 * n + o] = p21[j]; sout[5 * n + o] = p22[j];
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------

constexpr long long kMaxFloats = (1LL << 31) - 1;          // of one image tensor, stride included: every pixel index fits an int

int tv_levels(int H, int W, int scales, int min_side, int* hs, int* ws) {
    int L = 1;
    hs[0] = H; ws[0] = W;
    while (L < scales && L < kMaxLevels && (hs[L - 1] < ws[L - 1] ? hs[L - 1] : ws[L - 1]) / 2 >= min_side) {
        hs[L] = (hs[L - 1] + 1) / 2; ws[L] = (ws[L - 1] + 1) / 2;
        ++L;
    }
    return L;
}

size_t tv_align(size_t floats) { return (floats + 63) / 64 * 64; }                   // planes start on 256-byte boundaries

int tv_check_dims(const char* what, int B, int H, int W, int ps, int min_hw) {
    SN_REQUIRE(B >= 1 && B <= 65535, "%s: B must be 1..65535, got %d", what, B);
    SN_REQUIRE(H >= min_hw && W >= min_hw, "%s: H and W must be at least %d, got %d x %d", what, min_hw, H, W);
    SN_REQUIRE(ps >= 1, "%s: the pixel stride must be at least 1 float, got %d", what, ps);
    SN_REQUIRE((long long)B * H * W <= kMaxFloats / ps, "%s: %d x %d x %d pixels %d floats apart are more than 2^31 - 1 floats", what, B, H, W, ps);
    return STABNET_OK;
}

int tv_check_ptrs(const char* what, hipStream_t st, std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs) {
        if (!p) continue;
        char name[96];
        snprintf(name, sizeof name, "%s: a pointer", what);
        const int rc = sn_check_device(p, name, st);
        if (rc) return rc;
    }
    return STABNET_OK;
}

dim3 tv_grid(int H, int W, int B, int z = 1) { return dim3(cdiv((long)H * W, kThreads), B, z); }

int tv_down(const float* in, int ps, TvAff af, int B, int H, int W, float* out, hipStream_t st, Prof* prof) {
    const int h = (H + 1) / 2, w = (W + 1) / 2;
    const bool rec = prof && prof->begin(st);
    tvl1_down_kernel<<<tv_grid(h, w, B), kThreads, 0, st>>>(in, ps, af, H, W, out, h, w);
    if (rec) prof->end(st, PK_KERNEL_TVL1_DOWN, 0.0, 4.0 * B * ((double)H * W + (double)h * w));
    SN_LAUNCH_CHECK("tvl1_down_kernel");
    return STABNET_OK;
}

int tv_grad(const float* in, int ps, TvAff af, int B, int H, int W, float* gx, float* gy, hipStream_t st, Prof* prof) {
    const bool rec = prof && prof->begin(st);
    tvl1_grad_kernel<<<tv_grid(H, W, B), kThreads, 0, st>>>(in, ps, af, H, W, gx, gy);
    if (rec) prof->end(st, PK_KERNEL_TVL1_GRAD, 0.0, 12.0 * B * H * W);
    SN_LAUNCH_CHECK("tvl1_grad_kernel");
    return STABNET_OK;
}

int tv_warp(const float* i0, const float* i1, int ps, TvAff af, const float* gx, const float* gy, const float* u, float* cst, int B, int H, int W,
            hipStream_t st, Prof* prof) {
    const bool rec = prof && prof->begin(st);
    tvl1_warp_kernel<<<tv_grid(H, W, B), kThreads, 0, st>>>(i0, i1, ps, af, gx, gy, u, cst, (size_t)B * H * W, H, W);
    if (rec) prof->end(st, PK_KERNEL_TVL1_WARP, 0.0, 40.0 * B * H * W);            // I0, I1, I1x, I1y, u1, u2 read once each, four planes written
    SN_LAUNCH_CHECK("tvl1_warp_kernel");
    return STABNET_OK;
}

int tv_up(const float* in, int B, int h, int w, float* out, int H, int W, hipStream_t st, Prof* prof) {
    const bool rec = prof && prof->begin(st);
    tvl1_up_kernel<<<tv_grid(H, W, B, 2), kThreads, 0, st>>>(in, h, w, out, H, W, B);
    if (rec) prof->end(st, PK_KERNEL_TVL1_UP, 0.0, 8.0 * B * ((double)H * W + (double)h * w));
    SN_LAUNCH_CHECK("tvl1_up_kernel");
    return STABNET_OK;
}

int tv_map(const float* u, int B, int H, int W, float* uv, float* map, hipStream_t st, Prof* prof) {
    const bool rec = prof && prof->begin(st);
    tvl1_map_kernel<<<tv_grid(H, W, B), kThreads, 0, st>>>(u, (size_t)B * H * W, uv, map, H, W);
    if (rec) prof->end(st, PK_KERNEL_TVL1_MAP, 0.0, 8.0 * B * H * W * (1 + (uv != nullptr) + (map != nullptr)));
    SN_LAUNCH_CHECK("tvl1_map_kernel");
    return STABNET_OK;
}

// n sweeps from *cur into *oth and back again; on return *cur names the buffer that holds the result.
int tv_iterate(float** cur, float** oth, const float* cst, int B, int H, int W, float lt, float taut, float theta, int n, bool fused,
               hipStream_t st, Prof* prof) {
    const size_t pl = (size_t)B * H * W;
    const double bytes = 64.0 * pl;                                                 // ten planes read, six written: the least a launch moves
    for (int done = 0; done < n;) {
        const int k = fused ? (n - done < kK ? n - done : kK) : 1;
        const bool rec = prof && prof->begin(st);
        if (fused)
            tvl1_fused_kernel<<<dim3(cdiv(W, kTX), cdiv(H, kTY), B), kFThreads, 0, st>>>(*cur, *oth, cst, pl, H, W, lt, taut, theta, k);
        else
            tvl1_step_kernel<<<dim3(cdiv(W, kSX), cdiv(H, kSY), B), kThreads, 0, st>>>(*cur, *oth, cst, pl, H, W, lt, taut, theta);
        if (rec) prof->end(st, fused ? PK_KERNEL_TVL1_FUSED : PK_KERNEL_TVL1_STEP, 0.0, bytes, k);
        SN_LAUNCH_CHECK(fused ? "tvl1_fused_kernel" : "tvl1_step_kernel");
        float* t = *cur; *cur = *oth; *oth = t;
        done += k;
    }
    return STABNET_OK;
}

int tv_check_params(const char* what, float tau, float lambda, float theta) {
    SN_REQUIRE(tau > 0.0f && lambda > 0.0f && theta > 0.0f && tau < INFINITY && lambda < INFINITY && theta < INFINITY,
               "%s: tau, lambda and theta must be positive and finite, got %g %g %g", what, tau, lambda, theta);
    return STABNET_OK;
}

bool tv_fused_default() {
    const char* e = getenv("STABNET_TVL1_FUSED");                                   // A/B switch: 0 = one launch per sweep
    return !(e && e[0] == '0' && e[1] == 0);
}

}  // namespace

// ---- what csrc/klt.hip shares (tvl1_shared.h) ------------------------------------------------------------------------------------------

int sn_tv_levels(int H, int W, int scales, int min_side, int* hs, int* ws) { return tv_levels(H, W, scales, min_side, hs, ws); }

int sn_tv_down(const float* in, int ps, float off, float scl, int on, int B, int H, int W, float* out, hipStream_t st, Prof* prof) {
    return tv_down(in, ps, TvAff{off, scl, on}, B, H, W, out, st, prof);
}

int sn_tv_grad(const float* in, int ps, float off, float scl, int on, int B, int H, int W, float* gx, float* gy, hipStream_t st, Prof* prof) {
    return tv_grad(in, ps, TvAff{off, scl, on}, B, H, W, gx, gy, st, prof);
}

#define TV_TRY(call) do { const int rc__ = (call); if (rc__) return rc__; } while (0)

extern "C" {

/* See include/stabnet_hip.h. */
int stabnet_tvl1_levels(int H, int W, int scales, int min_side, int* hw) {
    int hs[kMaxLevels], ws[kMaxLevels];
    if (H < 2 || W < 2 || scales < 1 || min_side < 2) {
        stabnet_set_error("tvl1_levels: H, W >= 2, scales >= 1, min_side >= 2 wanted, got %d x %d, %d, %d", H, W, scales, min_side);
        return STABNET_ERR_BAD_ARG;
    }
    const int L = tv_levels(H, W, scales, min_side, hs, ws);
    for (int l = 0; hw && l < L; ++l) { hw[2 * l] = hs[l]; hw[2 * l + 1] = ws[l]; }
    return L;
}

void stabnet_tvl1_fused_geometry(int* k_tx_ty) {
    if (k_tx_ty) { k_tx_ty[0] = kK; k_tx_ty[1] = kTX; k_tx_ty[2] = kTY; }
}

size_t stabnet_tvl1_workspace_bytes(int B, int H, int W, int scales, int min_side) {
    if (B < 1 || B > 65535 || H < 8 || W < 8 || scales < 1 || min_side < 2 || (long long)B * H * W > kMaxFloats) return 0;
    int hs[kMaxLevels], ws[kMaxLevels];
    const int L = tv_levels(H, W, scales, min_side, hs, ws);
    size_t f = 18 * tv_align((size_t)B * H * W);                                    // I1x, I1y, four constants, two states of six planes
    for (int l = 1; l < L; ++l) f += 2 * tv_align((size_t)B * hs[l] * ws[l]);      // the coarser levels of I0 and I1
    return f * sizeof(float);
}

int stabnet_tvl1_pyramid_down(const float* in, int pixel_stride, int B, int H, int W, float* out, void* stream, void* prof) {
    SN_REQUIRE(in && out, "tvl1_pyramid_down: null pointer");
    TV_TRY(tv_check_dims("tvl1_pyramid_down", B, H, W, pixel_stride, 2));
    TV_TRY(tv_check_ptrs("tvl1_pyramid_down", (hipStream_t)stream, {in, out}));
    return tv_down(in, pixel_stride, TvAff{0.0f, 1.0f, 0}, B, H, W, out, (hipStream_t)stream, static_cast<Prof*>(prof));
}

int stabnet_tvl1_gradient(const float* in, int pixel_stride, int B, int H, int W, float* gx, float* gy, void* stream, void* prof) {
    SN_REQUIRE(in && gx && gy, "tvl1_gradient: null pointer");
    TV_TRY(tv_check_dims("tvl1_gradient", B, H, W, pixel_stride, 2));
    TV_TRY(tv_check_ptrs("tvl1_gradient", (hipStream_t)stream, {in, gx, gy}));
    return tv_grad(in, pixel_stride, TvAff{0.0f, 1.0f, 0}, B, H, W, gx, gy, (hipStream_t)stream, static_cast<Prof*>(prof));
}

int stabnet_tvl1_warp(const float* i0, const float* i1, int pixel_stride, const float* gx, const float* gy, const float* u, float* consts,
                      int B, int H, int W, void* stream, void* prof) {
    SN_REQUIRE(i0 && i1 && gx && gy && u && consts, "tvl1_warp: null pointer");
    TV_TRY(tv_check_dims("tvl1_warp", B, H, W, pixel_stride, 2));
    TV_TRY(tv_check_ptrs("tvl1_warp", (hipStream_t)stream, {i0, i1, gx, gy, u, consts}));
    return tv_warp(i0, i1, pixel_stride, TvAff{0.0f, 1.0f, 0}, gx, gy, u, consts, B, H, W, (hipStream_t)stream, static_cast<Prof*>(prof));
}

int stabnet_tvl1_upsample(const float* u_coarse, int B, int h, int w, float* u_fine, int H, int W, void* stream, void* prof) {
    SN_REQUIRE(u_coarse && u_fine, "tvl1_upsample: null pointer");
    TV_TRY(tv_check_dims("tvl1_upsample", B, H, W, 1, 2));
    SN_REQUIRE(h == (H + 1) / 2 && w == (W + 1) / 2, "tvl1_upsample: the coarse level of %d x %d is %d x %d, got %d x %d", H, W, (H + 1) / 2,
               (W + 1) / 2, h, w);
    TV_TRY(tv_check_ptrs("tvl1_upsample", (hipStream_t)stream, {u_coarse, u_fine}));
    return tv_up(u_coarse, B, h, w, u_fine, H, W, (hipStream_t)stream, static_cast<Prof*>(prof));
}

int stabnet_tvl1_flow_to_map(const float* u, int B, int H, int W, float* uv_out, float* map_out, void* stream, void* prof) {
    SN_REQUIRE(u && (uv_out || map_out), "tvl1_flow_to_map: null pointer (u, or both outputs)");
    TV_TRY(tv_check_dims("tvl1_flow_to_map", B, H, W, 2, 2));
    TV_TRY(tv_check_ptrs("tvl1_flow_to_map", (hipStream_t)stream, {u, uv_out, map_out}));
    return tv_map(u, B, H, W, uv_out, map_out, (hipStream_t)stream, static_cast<Prof*>(prof));
}

int stabnet_tvl1_iterate(float* state, float* scratch, const float* consts, int B, int H, int W, float tau, float lambda, float theta, int n,
                         int fused, void* stream, void* prof) {
    SN_REQUIRE(state && scratch && consts, "tvl1_iterate: null pointer");
    SN_REQUIRE(state != scratch, "tvl1_iterate: state and scratch are the same buffer");
    TV_TRY(tv_check_dims("tvl1_iterate", B, H, W, 6, 2));
    TV_TRY(tv_check_params("tvl1_iterate", tau, lambda, theta));
    SN_REQUIRE(n >= 1 && n <= 1 << 20, "tvl1_iterate: n must be 1..2^20, got %d", n);
    SN_REQUIRE(fused == 0 || fused == 1, "tvl1_iterate: fused must be 0 (one launch per iteration) or 1, got %d", fused);
    hipStream_t st = (hipStream_t)stream;
    TV_TRY(tv_check_ptrs("tvl1_iterate", st, {state, scratch, consts}));
    float *cur = state, *oth = scratch;
    TV_TRY(tv_iterate(&cur, &oth, consts, B, H, W, lambda * theta, tau / theta, theta, n, fused != 0, st, static_cast<Prof*>(prof)));
    if (cur != state && hipMemcpyAsync(state, cur, 6 * (size_t)B * H * W * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
        stabnet_set_error("tvl1_iterate: copying the result back failed: %s", hipGetErrorString(hipGetLastError()));
        return STABNET_ERR_LAUNCH;
    }
    return STABNET_OK;
}

int stabnet_tvl1_flow(const float* i0, const float* i1, int pixel_stride, float in_offset, float in_scale, int B, int H, int W, float tau, float lambda, float theta,
                      int scales, int warps, int iters, int min_side, void* workspace, size_t workspace_bytes, float* uv_out,
                      float* map_out, void* stream, void* profp) {
    SN_REQUIRE(i0 && i1 && workspace, "tvl1_flow: null pointer");
    SN_REQUIRE(uv_out || map_out, "tvl1_flow: both outputs are null");
    TV_TRY(tv_check_dims("tvl1_flow", B, H, W, pixel_stride, 8));
    TV_TRY(tv_check_params("tvl1_flow", tau, lambda, theta));
    SN_REQUIRE(in_offset > -INFINITY && in_offset < INFINITY && in_scale > 0.0f && in_scale < INFINITY,
               "tvl1_flow: in_offset must be finite and in_scale positive and finite, got %g %g", in_offset, in_scale);
    SN_REQUIRE(scales >= 1 && warps >= 1 && iters >= 1, "tvl1_flow: scales, warps and iters must be at least 1, got %d %d %d", scales, warps, iters);
    SN_REQUIRE(warps <= 1 << 10 && iters <= 1 << 20, "tvl1_flow: at most 2^10 warps of 2^20 iterations, got %d %d", warps, iters);
    SN_REQUIRE(min_side >= 2, "tvl1_flow: min_side must be at least 2, got %d", min_side);
    const size_t need = stabnet_tvl1_workspace_bytes(B, H, W, scales, min_side);
    SN_REQUIRE(need != 0 && workspace_bytes >= need, "tvl1_flow: the workspace holds %zu bytes, %zu are needed", workspace_bytes, need);
    SN_REQUIRE(((uintptr_t)workspace & 15) == 0, "tvl1_flow: the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    TV_TRY(tv_check_ptrs("tvl1_flow", st, {i0, i1, workspace, uv_out, map_out}));
    Prof* prof = static_cast<Prof*>(profp);
    const bool fused = tv_fused_default();
    const float lt = lambda * theta, taut = tau / theta;

    int hs[kMaxLevels], ws[kMaxLevels];
    const int L = tv_levels(H, W, scales, min_side, hs, ws);
    const size_t n0 = tv_align((size_t)B * H * W);
    float* base = static_cast<float*>(workspace);
    float *gx = base, *gy = base + n0, *cst = base + 2 * n0, *sa = base + 6 * n0, *sb = base + 12 * n0;
    const float *p0[kMaxLevels], *p1[kMaxLevels];
    int ps[kMaxLevels];
    const TvAff none = {0.0f, 1.0f, 0}, first = {in_offset, in_scale, !(in_offset == 0.0f && in_scale == 1.0f)};
    p0[0] = i0; p1[0] = i1; ps[0] = pixel_stride;
    float* next = base + 18 * n0;
    for (int l = 1; l < L; ++l) {
        const size_t nl = tv_align((size_t)B * hs[l] * ws[l]);
        TV_TRY(tv_down(p0[l - 1], ps[l - 1], l == 1 ? first : none, B, hs[l - 1], ws[l - 1], next, st, prof));
        TV_TRY(tv_down(p1[l - 1], ps[l - 1], l == 1 ? first : none, B, hs[l - 1], ws[l - 1], next + nl, st, prof));
        p0[l] = next; p1[l] = next + nl; ps[l] = 1;
        next += 2 * nl;
    }
    float *cur = sa, *oth = sb;
    for (int l = L - 1; l >= 0; --l) {
        const int h = hs[l], w = ws[l];
        const size_t pl = (size_t)B * h * w;
        hipError_t e;
        if (l == L - 1) {
            e = hipMemsetAsync(cur, 0, 6 * pl * sizeof(float), st);                 // u = 0, p = 0
        } else {
            TV_TRY(tv_up(cur, B, hs[l + 1], ws[l + 1], oth, h, w, st, prof));       // u of the coarser level, held as [2][B][h'][w'] in cur
            float* t = cur; cur = oth; oth = t;
            e = hipMemsetAsync(cur + 2 * pl, 0, 4 * pl * sizeof(float), st);        // the duals start at 0 at every level
        }
        if (e != hipSuccess) {
            stabnet_set_error("tvl1_flow: hipMemsetAsync failed: %s", hipGetErrorString(e));
            return STABNET_ERR_LAUNCH;
        }
        TV_TRY(tv_grad(p1[l], ps[l], l == 0 ? first : none, B, h, w, gx, gy, st, prof));
        for (int wi = 0; wi < warps; ++wi) {
            TV_TRY(tv_warp(p0[l], p1[l], ps[l], l == 0 ? first : none, gx, gy, cur, cst, B, h, w, st, prof));
            TV_TRY(tv_iterate(&cur, &oth, cst, B, h, w, lt, taut, theta, iters, fused, st, prof));
        }
    }
    return tv_map(cur, B, H, W, uv_out, map_out, st, prof);
}

}  // extern "C"
