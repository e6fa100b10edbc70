// Feature matches for the records' feature_matches1 / 2: Shi-Tomasi corners, one per grid cell, tracked from i0 to i1 by pyramidal
// Lucas-Kanade with a FIXED number of iterations and kept when the track back from i1 to i0 returns to where it started.
// tests/klt_model.py is the same arithmetic in NumPy and the yardstick: every operation below is one explicitly rounded float32
// operation (__fadd_rn, __fmul_rn, __fdiv_rn, sqrtf), in the model's order, and the library is built with -ffp-contract=off.
// The pyramid, the centred-difference gradient and the bilinear sample are TV-L1's (tvl1_shared.h): the same kernels and the same
// device function, not a restatement.  include/stabnet_hip.h states the operation order.
//
//   detect  klt_detect_kernel, one workgroup per cell: 16 x 16 sub-tiles of the cell with a halo of r + 1 go through LDS; gradient
//           products, the two box-sum passes and the response stay on chip; every thread keeps its best (response, linear index),
//           a butterfly of __shfl_xor and four LDS slots reduce them, ties to the smaller index at every step.  The response plane
//           is written only when the stage entry point asks for it.
//   track   klt_track_kernel, the hot path: one wave per point, four points per workgroup, forward and backward track in the same
//           wave.  Lane l owns the window samples l, l + 64, l + 128, l + 192 (those below (2R+1)^2 <= 225); their template values
//           T, Tx, Ty (12 floats) stay in registers over the iterations of a level.  Window sums: the lane adds its samples in that
//           order, starting from 0, then six butterfly steps (partner distances 32, 16, 8, 4, 2, 1, v = v + partner's v): float
//           addition commutes bitwise, so all 64 lanes end with the same bits and take the same branch-free update.  No LDS, no
//           barrier: the four waves of a workgroup are independent.  A lost point's arithmetic goes on (the sample clamps its
//           coordinates and maps NaN to 0), so no lane diverges and nothing reads out of bounds.
//   finish  klt_finish_kernel, one workgroup per image: the largest response (a max over the cells' maxima: exact in any order),
//           the detected / valid flags, an integer prefix scan over the cells (ballot + popcount per wave, four partial counts in
//           LDS) that compacts the rows in cell order, zeros from row n on.
// No atomics, no allocation, no host copy, nothing read back: the whole solve sits on one stream and can be captured in a graph.
#include <climits>
#include <cmath>
#include <cstring>
#include <initializer_list>

#include "common.h"
#include "prof.h"
#include "tvl1_shared.h"

namespace {

constexpr int kThreads = 256, kWave = 64, kPointsPerWg = kThreads / kWave;
constexpr int kDT = 16;                                    // detection sub-tile: kDT * kDT = kThreads pixels
constexpr int kMaxBoxR = 4, kMaxWinR = 7;                  // box radius r (LDS tile), window radius R ((2R+1)^2 <= 4 * 64 samples)
constexpr int kDI = kDT + 2 * (kMaxBoxR + 1), kDP = kDT + 2 * kMaxBoxR;
constexpr int kLevels = 8, kTvLevels = 16;
constexpr long long kMaxFloats = (1LL << 31) - 1;
static_assert(kDT * kDT == kThreads && (2 * kMaxWinR + 1) * (2 * kMaxWinR + 1) <= 4 * kWave, "tile and window");

// 0.5 * ((a + c) - sqrt((a - c)^2 + 4 * (b * b))): the smaller eigenvalue of [[a, b], [b, c]]
__device__ __forceinline__ float klt_min_eig(float a, float b, float c) {
    const float d = __fsub_rn(a, c);
    return __fmul_rn(0.5f, __fsub_rn(__fadd_rn(a, c), sqrtf(__fadd_rn(__fmul_rn(d, d), __fmul_rn(4.0f, __fmul_rn(b, b))))));
}

__device__ __forceinline__ bool klt_better(float r, int i, float best, int bi) { return r > best || (r == best && i < bi); }

// ---- detection: grid (cells along x, cells along y, B) --------------------------------------------------------------------------------
// cand [B][cells][4] = x, y, response, 0 (klt_finish_kernel sets the flag); plane [B][H][W] (or null): the response itself.
// border >= r + 1 (checked by the host): no pixel that keeps its response has a box or a gradient that leaves the image; the
// clamped loads only keep the reads of the others inside it.
__global__ __launch_bounds__(kThreads) void klt_detect_kernel(const float* __restrict__ i0, int ps, TvAff af, int H, int W, int r, int border,
                                                              int cell, float4* __restrict__ cand, float* __restrict__ plane) {
    __shared__ float sI[kDI * kDI], sP[3][kDP * kDP], sX[3][kDP * kDT];
    __shared__ float sBest[kPointsPerWg];
    __shared__ int sIdx[kPointsPerWg];
    const int X0 = blockIdx.x * cell, Y0 = blockIdx.y * cell, X1 = X0 + cell < W ? X0 + cell : W, Y1 = Y0 + cell < H ? Y0 + cell : H;
    const float* img = i0 + (size_t)blockIdx.z * H * W * ps;
    const int tid = threadIdx.x, tx = tid % kDT, ty = tid / kDT, ni = kDT + 2 * (r + 1), np = kDT + 2 * r;
    float best = -INFINITY;
    int bidx = Y0 * W + X0;
    for (int y0 = Y0; y0 < Y1; y0 += kDT)
        for (int x0 = X0; x0 < X1; x0 += kDT) {
            for (int l = tid; l < ni * ni; l += kThreads) {
                const int iy = l / ni, ix = l - iy * ni;
                int y = y0 - (r + 1) + iy, x = x0 - (r + 1) + ix;
                y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
                x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
                sI[iy * kDI + ix] = tv_px(img[((size_t)y * W + x) * ps], af);
            }
            __syncthreads();
            for (int l = tid; l < np * np; l += kThreads) {                         // pixel (y0 - r + py, x0 - r + px) = tile (py + 1, px + 1)
                const int py = l / np, px = l - py * np;
                const float gx = __fmul_rn(0.5f, __fsub_rn(sI[(py + 1) * kDI + px + 2], sI[(py + 1) * kDI + px]));
                const float gy = __fmul_rn(0.5f, __fsub_rn(sI[(py + 2) * kDI + px + 1], sI[py * kDI + px + 1]));
                sP[0][py * kDP + px] = __fmul_rn(gx, gx);
                sP[1][py * kDP + px] = __fmul_rn(gx, gy);
                sP[2][py * kDP + px] = __fmul_rn(gy, gy);
            }
            __syncthreads();
            for (int l = tid; l < np * kDT; l += kThreads) {                        // along x, left to right
                const int py = l / kDT, c = l - py * kDT;
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    float v = sP[p][py * kDP + c];
                    for (int k = 1; k <= 2 * r; ++k) v = __fadd_rn(v, sP[p][py * kDP + c + k]);
                    sX[p][py * kDT + c] = v;
                }
            }
            __syncthreads();
            float s[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) {                                           // along y, top to bottom
                float v = sX[p][ty * kDT + tx];
                for (int k = 1; k <= 2 * r; ++k) v = __fadd_rn(v, sX[p][(ty + k) * kDT + tx]);
                s[p] = v;
            }
            const int x = x0 + tx, y = y0 + ty;
            const bool inner = x >= border && x < W - border && y >= border && y < H - border;
            const float resp = inner ? klt_min_eig(s[0], s[1], s[2]) : 0.0f;
            if (x < X1 && y < Y1) {
                const int idx = y * W + x;
                if (plane) plane[(size_t)blockIdx.z * H * W + idx] = resp;
                if (klt_better(resp, idx, best, bidx)) { best = resp; bidx = idx; }
            }
        }                                                                           // (the next tile's stores follow two barriers)
    if (!cand) return;
#pragma unroll
    for (int d = kWave / 2; d; d >>= 1) {
        const float ob = __shfl_xor(best, d);
        const int oi = __shfl_xor(bidx, d);
        if (klt_better(ob, oi, best, bidx)) { best = ob; bidx = oi; }
    }
    if ((tid & (kWave - 1)) == 0) { sBest[tid / kWave] = best; sIdx[tid / kWave] = bidx; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kPointsPerWg; ++w)
            if (klt_better(sBest[w], sIdx[w], best, bidx)) { best = sBest[w]; bidx = sIdx[w]; }
        const int y = bidx / W, x = bidx - y * W;
        cand[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = make_float4((float)x, (float)y, best, 0.0f);
    }
}

// ---- tracking: grid (cdiv(N, 4), B), one wave per point -------------------------------------------------------------------------------

// a, b: level l of i0 and i1 ([B][h][w], pixels psa / psb floats apart); ax .. by: their gradients (dense)
struct KltLevel { const float *a, *b, *ax, *ay, *bx, *by; int h, w, psa, psb; };
struct KltPyr { KltLevel lv[kLevels]; int L; TvAff af; };              // af: how level 0 is read

__device__ __forceinline__ float klt_wsum(float v) {
#pragma unroll
    for (int d = kWave / 2; d; d >>= 1) v = __fadd_rn(v, __shfl_xor(v, d));
    return v;
}

// One direction, coarse to fine: from (px0, py0) in image `dir` (0: i0, 1: i1) to (qx, qy) in the other one.
__device__ __forceinline__ void klt_track_dir(const KltPyr& P, int dir, int img, float px0, float py0, int R, int iters, float min_eig,
                                              int lane, float& qx, float& qy, bool& lost) {
    const int side = 2 * R + 1, n = side * side;
    const TvAff none = {0.0f, 1.0f, 0};
    float ox[4], oy[4];
    bool valid[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int s = lane + kWave * k, row = s / side;
        valid[k] = s < n;
        oy[k] = (float)(row - R);
        ox[k] = (float)(s - row * side - R);
    }
    float dx = 0.0f, dy = 0.0f;
    qx = px0; qy = py0;
    for (int l = P.L - 1; l >= 0; --l) {
        const KltLevel& V = P.lv[l];
        const int h = V.h, w = V.w, psA = dir ? V.psb : V.psa, psB = dir ? V.psa : V.psb;
        const size_t hw = (size_t)h * w;
        const float* A = (dir ? V.b : V.a) + img * hw * psA;
        const float* Bm = (dir ? V.a : V.b) + img * hw * psB;
        const float* Ax = (dir ? V.bx : V.ax) + img * hw;
        const float* Ay = (dir ? V.by : V.ay) + img * hw;
        const TvAff af = l == 0 ? P.af : none;
        const float sc = __int_as_float((127 - l) << 23);                           // 2^-l
        const float pxl = __fmul_rn(px0, sc), pyl = __fmul_rn(py0, sc);
        float x[4], y[4], T[4], Tx[4], Ty[4];
        float sa = 0.0f, sb = 0.0f, scc = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x[k] = __fadd_rn(pxl, ox[k]);
            y[k] = __fadd_rn(pyl, oy[k]);
            T[k] = tv_bilinear(A, psA, h, w, y[k], x[k], af);
            Tx[k] = tv_bilinear(Ax, 1, h, w, y[k], x[k], none);
            Ty[k] = tv_bilinear(Ay, 1, h, w, y[k], x[k], none);
            const float na = __fadd_rn(sa, __fmul_rn(Tx[k], Tx[k])), nb = __fadd_rn(sb, __fmul_rn(Tx[k], Ty[k])),
                        nc = __fadd_rn(scc, __fmul_rn(Ty[k], Ty[k]));
            sa = valid[k] ? na : sa;
            sb = valid[k] ? nb : sb;
            scc = valid[k] ? nc : scc;
        }
        const float a = klt_wsum(sa), b = klt_wsum(sb), c = klt_wsum(scc);
        const float det = __fsub_rn(__fmul_rn(a, c), __fmul_rn(b, b));
        lost = lost || __fdiv_rn(klt_min_eig(a, b, c), (float)n) < min_eig || det == 0.0f;
        for (int it = 0; it < iters; ++it) {
            float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float e = __fsub_rn(T[k], tv_bilinear(Bm, psB, h, w, __fadd_rn(y[k], dy), __fadd_rn(x[k], dx), af));
                const float n1 = __fadd_rn(s1, __fmul_rn(e, Tx[k])), n2 = __fadd_rn(s2, __fmul_rn(e, Ty[k]));
                s1 = valid[k] ? n1 : s1;
                s2 = valid[k] ? n2 : s2;
            }
            const float bx = klt_wsum(s1), by = klt_wsum(s2);
            dx = __fadd_rn(dx, __fdiv_rn(__fsub_rn(__fmul_rn(c, bx), __fmul_rn(b, by)), det));
            dy = __fadd_rn(dy, __fdiv_rn(__fsub_rn(__fmul_rn(a, by), __fmul_rn(b, bx)), det));
        }
        qx = __fadd_rn(pxl, dx);
        qy = __fadd_rn(pyl, dy);
        lost = lost || !(qx >= 0.0f && qx <= (float)(w - 1) && qy >= 0.0f && qy <= (float)(h - 1));     // (false for NaN: lost)
        if (l) { dx = __fmul_rn(2.0f, dx); dy = __fmul_rn(2.0f, dy); }
    }
}

// pts: point j of image b at pts[(b * N + j) * pstride] = x, + 1 = y.  trk [B][N][4] = qx, qy, lost, |p' - p|^2; lost: 0, 0, 1, 0.
__global__ __launch_bounds__(kThreads) void klt_track_kernel(KltPyr P, const float* __restrict__ pts, int pstride, int N, int R, int iters,
                                                             float min_eig, float4* __restrict__ trk) {
    const int lane = threadIdx.x & (kWave - 1), pt = blockIdx.x * kPointsPerWg + threadIdx.x / kWave, img = blockIdx.y;
    if (pt >= N) return;                                                            // the whole wave
    const size_t o = (size_t)img * N + pt;
    const float px = pts[o * pstride], py = pts[o * pstride + 1];
    float qx, qy, rx, ry;
    bool lost = false;
    klt_track_dir(P, 0, img, px, py, R, iters, min_eig, lane, qx, qy, lost);
    klt_track_dir(P, 1, img, qx, qy, R, iters, min_eig, lane, rx, ry, lost);
    const float ex = __fsub_rn(rx, px), ey = __fsub_rn(ry, py);
    const float fb2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
    if (lane == 0) trk[o] = lost ? make_float4(0.0f, 0.0f, 1.0f, 0.0f) : make_float4(qx, qy, 0.0f, fb2);
}

// ---- finish: grid (B), one workgroup per image ----------------------------------------------------------------------------------------
// cand[.].w = detected, always; with trk: the rows of the valid matches in cell order, at most maxm - 1, zeros from row n on, n.
__global__ __launch_bounds__(kThreads) void klt_finish_kernel(float4* __restrict__ cand, const float4* __restrict__ trk, int nc, float floor_,
                                                              float quality, float fb2max, int H, int W, int maxm,
                                                              float4* __restrict__ rows, int* __restrict__ count) {
    __shared__ float sMax[kPointsPerWg];
    __shared__ int sCnt[kPointsPerWg];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    float4* cd = cand + (size_t)blockIdx.x * nc;
    float top = -INFINITY;
    for (int i = tid; i < nc; i += kThreads) top = fmaxf(top, cd[i].z);
#pragma unroll
    for (int d = kWave / 2; d; d >>= 1) top = fmaxf(top, __shfl_xor(top, d));
    if (lane == 0) sMax[wave] = top;
    __syncthreads();
    top = fmaxf(fmaxf(sMax[0], sMax[1]), fmaxf(sMax[2], sMax[3]));
    const float bar = __fmul_rn(quality, top);
    int base = 0;
    for (int i0 = 0; i0 < nc; i0 += kThreads) {                                     // (uniform trip count: the barriers are safe)
        const int i = i0 + tid;
        bool ok = false;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), t = c;
        if (i < nc) {
            c = cd[i];
            const bool det = c.z > 0.0f && c.z >= floor_ && c.z >= bar;
            cd[i].w = det ? 1.0f : 0.0f;
            if (trk) {
                t = trk[(size_t)blockIdx.x * nc + i];
                ok = det && t.z == 0.0f && t.w <= fb2max;
            }
        }
        if (!trk) continue;
        const unsigned long long m = __ballot(ok);
        if (lane == 0) sCnt[wave] = __popcll(m);
        __syncthreads();
        int pos = base + __popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) pos += sCnt[w];
        if (ok && pos < maxm - 1)
            rows[(size_t)blockIdx.x * maxm + pos] =
                make_float4(__fsub_rn(__fdiv_rn(__fmul_rn(2.0f, c.x), (float)W), 1.0f), __fsub_rn(__fdiv_rn(__fmul_rn(2.0f, c.y), (float)H), 1.0f),
                            __fsub_rn(__fdiv_rn(__fmul_rn(2.0f, t.x), (float)W), 1.0f), __fsub_rn(__fdiv_rn(__fmul_rn(2.0f, t.y), (float)H), 1.0f));
        base += sCnt[0] + sCnt[1] + sCnt[2] + sCnt[3];
        __syncthreads();                                                            // sCnt is written again in the next round
    }
    if (!trk) return;
    const int n = base < maxm - 1 ? base : maxm - 1;
    for (int i = n + tid; i < maxm; i += kThreads) rows[(size_t)blockIdx.x * maxm + i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (tid == 0) count[blockIdx.x] = n;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------

size_t kl_align(size_t floats) { return (floats + 63) / 64 * 64; }

struct KltGeom { int L, hs[kTvLevels], ws[kTvLevels]; size_t pyr_floats; };

KltGeom kl_geom(int B, int H, int W, int levels, int min_side) {
    KltGeom g;
    g.L = sn_tv_levels(H, W, levels, min_side, g.hs, g.ws);
    g.pyr_floats = 0;
    for (int l = 0; l < g.L; ++l) g.pyr_floats += (l ? 6 : 4) * kl_align((size_t)B * g.hs[l] * g.ws[l]);
    return g;
}

int kl_check_images(const char* what, int B, int H, int W, int ps0, int ps1, float off, float scl, int min_hw) {
    SN_REQUIRE(B >= 1 && B <= 65535, "%s: B must be 1..65535, got %d", what, B);
    SN_REQUIRE(H >= min_hw && W >= min_hw, "%s: H and W must be at least %d, got %d x %d", what, min_hw, H, W);
    SN_REQUIRE(ps0 >= 1 && ps1 >= 1, "%s: the pixel strides must be at least 1 float, got %d and %d", what, ps0, ps1);
    SN_REQUIRE((long long)B * H * W <= kMaxFloats / (ps0 > ps1 ? ps0 : ps1), "%s: %d x %d x %d pixels %d floats apart are more than 2^31 - 1 floats",
               what, B, H, W, ps0 > ps1 ? ps0 : ps1);
    SN_REQUIRE(off > -INFINITY && off < INFINITY && scl > 0.0f && scl < INFINITY,
               "%s: in_offset must be finite and in_scale positive and finite, got %g %g", what, off, scl);
    return STABNET_OK;
}

int kl_check_detect(const char* what, int H, int W, int r, int border, int cell, float floor_, float quality) {
    SN_REQUIRE(r >= 1 && r <= kMaxBoxR, "%s: the box radius r must be 1..%d, got %d", what, kMaxBoxR, r);
    SN_REQUIRE(border >= r + 1 && border <= 1 << 20, "%s: border must be at least r + 1 = %d (no box may leave the image), got %d", what, r + 1, border);
    SN_REQUIRE(H >= 2 * border + 1 && W >= 2 * border + 1, "%s: H and W must be at least 2 * border + 1 = %d, got %d x %d", what, 2 * border + 1, H, W);
    SN_REQUIRE(cell >= 2 && cell <= 1 << 20, "%s: cell must be 2..2^20, got %d", what, cell);
    SN_REQUIRE(floor_ > 0.0f && floor_ < INFINITY && quality > 0.0f && quality < INFINITY,
               "%s: floor and quality must be positive and finite, got %g %g", what, floor_, quality);
    return STABNET_OK;
}

int kl_check_track(const char* what, int levels, int min_side, int R, int iters, float min_eig) {
    SN_REQUIRE(levels >= 1 && levels <= kLevels, "%s: levels must be 1..%d, got %d", what, kLevels, levels);
    SN_REQUIRE(min_side >= 2, "%s: min_side must be at least 2, got %d", what, min_side);
    SN_REQUIRE(R >= 1 && R <= kMaxWinR, "%s: the window radius R must be 1..%d (a lane owns four of the window's samples), got %d", what, kMaxWinR, R);
    SN_REQUIRE(iters >= 1 && iters <= 1 << 16, "%s: iters must be 1..2^16, got %d", what, iters);
    SN_REQUIRE(min_eig >= 0.0f && min_eig < INFINITY, "%s: min_eig must be finite and not negative, got %g", what, min_eig);
    return STABNET_OK;
}

int kl_check_ptrs(const char* what, hipStream_t st, std::initializer_list<const void*> ptrs) {
    char name[96];
    snprintf(name, sizeof name, "%s: a pointer", what);
    for (const void* p : ptrs) {
        const int rc = p ? sn_check_device(p, name, st) : STABNET_OK;
        if (rc) return rc;
    }
    return STABNET_OK;
}

#define KL_TRY(call) do { const int rc__ = (call); if (rc__) return rc__; } while (0)

int kl_detect(const float* i0, int ps, TvAff af, int B, int H, int W, int r, int border, int cell, float4* cand, float* plane, hipStream_t st,
              Prof* prof) {
    const bool rec = prof && prof->begin(st);
    klt_detect_kernel<<<dim3(cdiv(W, cell), cdiv(H, cell), B), kThreads, 0, st>>>(i0, ps, af, H, W, r, border, cell, cand, plane);
    if (rec) prof->end(st, PK_KERNEL_KLT_DETECT, 0.0, 4.0 * B * H * W * (plane ? 2 : 1));   // the image once (and the plane)
    SN_LAUNCH_CHECK("klt_detect_kernel");
    return STABNET_OK;
}

int kl_finish(float4* cand, const float4* trk, int B, int nc, float floor_, float quality, float fb, int H, int W, int maxm, float4* rows,
              int* count, hipStream_t st, Prof* prof) {
    const bool rec = prof && prof->begin(st);
    klt_finish_kernel<<<dim3(B), kThreads, 0, st>>>(cand, trk, nc, floor_, quality, fb * fb, H, W, maxm, rows, count);
    if (rec) prof->end(st, PK_KERNEL_KLT_FINISH, 0.0, 16.0 * B * (2.0 * nc + (trk ? nc + maxm : 0)));
    SN_LAUNCH_CHECK("klt_finish_kernel");
    return STABNET_OK;
}

// Pyramids and gradients of both images into the workspace, then one launch for every point of every image.
int kl_track(const float* i0, const float* i1, int ps0, int ps1, TvAff af, int B, int H, int W, const KltGeom& g, float* ws, const float* pts,
             int pstride, int N, int R, int iters, float min_eig, float4* trk, hipStream_t st, Prof* prof) {
    KltPyr P;
    memset(&P, 0, sizeof P);
    P.L = g.L;
    P.af = af;
    float* next = ws;
    for (int l = 0; l < g.L; ++l) {
        KltLevel& V = P.lv[l];
        const int h = g.hs[l], w = g.ws[l];
        const size_t nl = kl_align((size_t)B * h * w);
        V.h = h; V.w = w;
        if (l == 0) {
            V.a = i0; V.b = i1; V.psa = ps0; V.psb = ps1;
        } else {
            const KltLevel& U = P.lv[l - 1];
            const int on = l == 1 ? af.on : 0;
            KL_TRY(sn_tv_down(U.a, U.psa, af.off, af.scl, on, B, U.h, U.w, next, st, prof));
            KL_TRY(sn_tv_down(U.b, U.psb, af.off, af.scl, on, B, U.h, U.w, next + nl, st, prof));
            V.a = next; V.b = next + nl; V.psa = V.psb = 1;
            next += 2 * nl;
        }
        const int on = l == 0 ? af.on : 0;
        KL_TRY(sn_tv_grad(V.a, V.psa, af.off, af.scl, on, B, h, w, next, next + nl, st, prof));
        KL_TRY(sn_tv_grad(V.b, V.psb, af.off, af.scl, on, B, h, w, next + 2 * nl, next + 3 * nl, st, prof));
        V.ax = next; V.ay = next + nl; V.bx = next + 2 * nl; V.by = next + 3 * nl;
        next += 4 * nl;
    }
    const bool rec = prof && prof->begin(st);
    klt_track_kernel<<<dim3(cdiv(N, kPointsPerWg), B), kThreads, 0, st>>>(P, pts, pstride, N, R, iters, min_eig, trk);
    // bilinear taps: both directions, every level: three template planes and `iters` samples of the other image, four taps each
    if (rec) prof->end(st, PK_KERNEL_KLT_TRACK, 0.0, 16.0 * B * N * 2.0 * g.L * (3.0 + iters) * (2 * R + 1) * (2 * R + 1), iters);
    SN_LAUNCH_CHECK("klt_track_kernel");
    return STABNET_OK;
}

size_t kl_cell_floats(int B, int H, int W, int cell) { return kl_align(4 * (size_t)B * cdiv(H, cell) * cdiv(W, cell)); }

}  // namespace

extern "C" {

/* See include/stabnet_hip.h. */
int stabnet_klt_cells(int H, int W, int cell, int* rows_cols) {
    if (H < 1 || W < 1 || cell < 2) {
        stabnet_set_error("klt_cells: H, W >= 1 and cell >= 2 wanted, got %d x %d, %d", H, W, cell);
        return STABNET_ERR_BAD_ARG;
    }
    const long long ny = cdiv(H, cell), nx = cdiv(W, cell);
    if (ny * nx > INT_MAX) {
        stabnet_set_error("klt_cells: %lld x %lld cells are more than 2^31 - 1", ny, nx);
        return STABNET_ERR_BAD_ARG;
    }
    if (rows_cols) { rows_cols[0] = (int)ny; rows_cols[1] = (int)nx; }
    return (int)(ny * nx);
}

size_t stabnet_klt_workspace_bytes(int B, int H, int W, int levels, int min_side, int cell) {
    if (B < 1 || B > 65535 || H < 3 || W < 3 || levels < 1 || levels > kLevels || min_side < 2 || cell < 2 || (long long)B * H * W > kMaxFloats)
        return 0;
    return (kl_geom(B, H, W, levels, min_side).pyr_floats + 2 * kl_cell_floats(B, H, W, cell)) * sizeof(float);
}

int stabnet_klt_response(const float* i0, int pixel_stride, float in_offset, float in_scale, int B, int H, int W, int r, int border, float* resp,
                         void* stream, void* prof) {
    SN_REQUIRE(i0 && resp, "klt_response: null pointer");
    KL_TRY(kl_check_images("klt_response", B, H, W, pixel_stride, 1, in_offset, in_scale, 3));
    KL_TRY(kl_check_detect("klt_response", H, W, r, border, kDT, 1.0f, 1.0f));
    hipStream_t st = (hipStream_t)stream;
    KL_TRY(kl_check_ptrs("klt_response", st, {i0, resp}));
    const TvAff af = {in_offset, in_scale, !(in_offset == 0.0f && in_scale == 1.0f)};
    return kl_detect(i0, pixel_stride, af, B, H, W, r, border, kDT, nullptr, resp, st, static_cast<Prof*>(prof));
}

int stabnet_klt_detect(const float* i0, int pixel_stride, float in_offset, float in_scale, int B, int H, int W, int r, int border, int cell,
                       float floor, float quality, float* cand, void* stream, void* prof) {
    SN_REQUIRE(i0 && cand, "klt_detect: null pointer");
    KL_TRY(kl_check_images("klt_detect", B, H, W, pixel_stride, 1, in_offset, in_scale, 3));
    KL_TRY(kl_check_detect("klt_detect", H, W, r, border, cell, floor, quality));
    SN_REQUIRE(((uintptr_t)cand & 15) == 0, "klt_detect: cand must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    KL_TRY(kl_check_ptrs("klt_detect", st, {i0, cand}));
    const TvAff af = {in_offset, in_scale, !(in_offset == 0.0f && in_scale == 1.0f)};
    float4* cd = reinterpret_cast<float4*>(cand);
    KL_TRY(kl_detect(i0, pixel_stride, af, B, H, W, r, border, cell, cd, nullptr, st, static_cast<Prof*>(prof)));
    return kl_finish(cd, nullptr, B, cdiv(H, cell) * cdiv(W, cell), floor, quality, 0.0f, H, W, 2, nullptr, nullptr, st, static_cast<Prof*>(prof));
}

int stabnet_klt_track(const float* i0, const float* i1, int pixel_stride0, int pixel_stride1, float in_offset, float in_scale, int B, int H, int W,
                      const float* pts, int N, int levels, int min_side, int R, int iters, float min_eig, void* workspace, size_t workspace_bytes,
                      float* trk, void* stream, void* prof) {
    SN_REQUIRE(i0 && i1 && pts && workspace && trk, "klt_track: null pointer");
    KL_TRY(kl_check_images("klt_track", B, H, W, pixel_stride0, pixel_stride1, in_offset, in_scale, 3));
    KL_TRY(kl_check_track("klt_track", levels, min_side, R, iters, min_eig));
    SN_REQUIRE(N >= 1 && (long long)B * N <= kMaxFloats / 4, "klt_track: N must be at least 1 and B * N * 4 at most 2^31 - 1, got %d", N);
    const KltGeom g = kl_geom(B, H, W, levels, min_side);
    SN_REQUIRE(workspace_bytes >= g.pyr_floats * sizeof(float), "klt_track: the workspace holds %zu bytes, %zu are needed", workspace_bytes,
               g.pyr_floats * sizeof(float));
    SN_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)trk & 15) == 0, "klt_track: the workspace and trk must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    KL_TRY(kl_check_ptrs("klt_track", st, {i0, i1, pts, workspace, trk}));
    const TvAff af = {in_offset, in_scale, !(in_offset == 0.0f && in_scale == 1.0f)};
    return kl_track(i0, i1, pixel_stride0, pixel_stride1, af, B, H, W, g, static_cast<float*>(workspace), pts, 2, N, R, iters, min_eig,
                    reinterpret_cast<float4*>(trk), st, static_cast<Prof*>(prof));
}

int stabnet_klt_matches(const float* i0, const float* i1, int pixel_stride0, int pixel_stride1, float in_offset, float in_scale, int B, int H, int W,
                        int levels, int min_side, int r, int border, int cell, float floor, float quality, int R, int iters, float min_eig, float fb,
                        int max_matches, void* workspace, size_t workspace_bytes, float* matches, int* n, void* stream, void* profp) {
    SN_REQUIRE(i0 && i1 && workspace && matches && n, "klt_matches: null pointer");
    KL_TRY(kl_check_images("klt_matches", B, H, W, pixel_stride0, pixel_stride1, in_offset, in_scale, 3));
    KL_TRY(kl_check_detect("klt_matches", H, W, r, border, cell, floor, quality));
    KL_TRY(kl_check_track("klt_matches", levels, min_side, R, iters, min_eig));
    SN_REQUIRE(fb > 0.0f && fb < INFINITY, "klt_matches: fb must be positive and finite, got %g", fb);
    SN_REQUIRE(max_matches >= 2 && (long long)B * max_matches <= kMaxFloats / 4,
               "klt_matches: max_matches must be at least 2 (one row less is kept) and B * max_matches * 4 at most 2^31 - 1, got %d", max_matches);
    const long long nc = (long long)cdiv(H, cell) * cdiv(W, cell);
    SN_REQUIRE(B * nc <= kMaxFloats / 4, "klt_matches: %d x %lld cells are too many", B, nc);
    const size_t need = stabnet_klt_workspace_bytes(B, H, W, levels, min_side, cell);
    SN_REQUIRE(need != 0 && workspace_bytes >= need, "klt_matches: the workspace holds %zu bytes, %zu are needed", workspace_bytes, need);
    SN_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)matches & 15) == 0, "klt_matches: the workspace and matches must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    KL_TRY(kl_check_ptrs("klt_matches", st, {i0, i1, workspace, matches, n}));
    Prof* prof = static_cast<Prof*>(profp);
    const TvAff af = {in_offset, in_scale, !(in_offset == 0.0f && in_scale == 1.0f)};
    const KltGeom g = kl_geom(B, H, W, levels, min_side);
    float* base = static_cast<float*>(workspace);
    float4* cand = reinterpret_cast<float4*>(base + g.pyr_floats);
    float4* trk = reinterpret_cast<float4*>(base + g.pyr_floats + kl_cell_floats(B, H, W, cell));
    KL_TRY(kl_detect(i0, pixel_stride0, af, B, H, W, r, border, cell, cand, nullptr, st, prof));
    KL_TRY(kl_track(i0, i1, pixel_stride0, pixel_stride1, af, B, H, W, g, base, reinterpret_cast<const float*>(cand), 4, (int)nc, R, iters, min_eig,
                    trk, st, prof));
    return kl_finish(cand, trk, B, (int)nc, floor, quality, fb, H, W, max_matches, reinterpret_cast<float4*>(matches), n, st, prof);
}

}  // extern "C"
