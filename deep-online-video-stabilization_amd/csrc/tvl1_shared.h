// What csrc/tvl1.hip and csrc/klt.hip share: how a source image is read (pixel stride, offset and scale), the bilinear sample,
// and the host side of the pyramid and gradient launches (defined in tvl1.hip, so that both run the same kernels).
#pragma once
#include "common.h"
#include "prof.h"

#ifdef __HIPCC__
// what the solve reads from i0 / i1: (v + off) * scl, two rounded operations (a get_img channel to the 0..255 scale); on = 0: v itself
struct TvAff { float off, scl; int on; };
__device__ __forceinline__ float tv_px(float v, TvAff a) { return a.on ? __fmul_rn(__fadd_rn(v, a.off), a.scl) : v; }

// I (rows W * ps floats, pixels ps floats apart) at (y, x): coordinates clamped to [0, n-1], the upper neighbour to n-1
__device__ __forceinline__ float tv_bilinear(const float* __restrict__ I, int ps, int H, int W, float y, float x, TvAff af) {
    x = fminf(fmaxf(x, 0.0f), (float)(W - 1));
    y = fminf(fmaxf(y, 0.0f), (float)(H - 1));
    const float xf = floorf(x), yf = floorf(y);
    int x0 = (int)xf, y0 = (int)yf;
    x0 = x0 < 0 ? 0 : (x0 > W - 1 ? W - 1 : x0);                                    // (a NaN coordinate is the caller's error: it still reads inside)
    y0 = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0);
    const int x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;
    const float fx = __fsub_rn(x, xf), fy = __fsub_rn(y, yf);
    const float* r0 = I + (size_t)y0 * W * ps;
    const float* r1 = I + (size_t)y1 * W * ps;
    const float a = tv_px(r0[(size_t)x0 * ps], af), b = tv_px(r0[(size_t)x1 * ps], af), c = tv_px(r1[(size_t)x0 * ps], af), d = tv_px(r1[(size_t)x1 * ps], af);
    const float top = __fadd_rn(a, __fmul_rn(fx, __fsub_rn(b, a))), bot = __fadd_rn(c, __fmul_rn(fx, __fsub_rn(d, c)));
    return __fadd_rn(top, __fmul_rn(fy, __fsub_rn(bot, top)));
}
#endif

// levels of the pyramid: one more while there are fewer than `scales` (at most 16) and min(h, w) / 2 >= min_side; hs, ws [16]
int sn_tv_levels(int H, int W, int scales, int min_side, int* hs, int* ws);
// one level down / the centred-difference gradient of [B,H,W] images read as (v + off) * scl when `on` (else v itself)
int sn_tv_down(const float* in, int ps, float off, float scl, int on, int B, int H, int W, float* out, hipStream_t st, Prof* prof);
int sn_tv_grad(const float* in, int ps, float off, float scl, int on, int B, int H, int W, float* gx, float* gy, hipStream_t st, Prof* prof);
