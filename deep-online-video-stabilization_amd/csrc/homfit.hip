// Robust homography fit over a batch of match lists, as stabnet_klt_matches writes them: RANSAC with a fixed number of hypotheses, a
// float64 least-squares refit over the winner's inliers, and the final mask.  tests/homfit_model.py is the same arithmetic in NumPy
// and the yardstick: every float operation below is one explicitly rounded operation (__fadd_rn, __fmul_rn, __fdiv_rn; __dadd_rn,
// __dmul_rn, __ddiv_rn, __dsqrt_rn), in the model's order, and the library is built with -ffp-contract=off.  include/stabnet_hip.h
// states the operation order.
//
//   homfit_kernel, one workgroup of 256 threads per pair.  The pair's n rows are staged once in LDS (16 bytes a row, at most 16 KiB).
//   sample  thread t owns the hypotheses t, t + 256, ...: four distinct row indices from a chain of 32-bit mixes, uint32 only.
//   model   the four-point homography through the projective basis: two adjugates of matrices whose last row is 1 1 1, one product,
//           eight divisions.  Branch-free, no pivoting; a non-finite entry makes the hypothesis invalid.
//   score   every lane reads the same LDS row (a broadcast) and counts the rows its model maps within thr_px; a thread keeps its
//           best (count, k), a butterfly of __shfl_xor and four LDS slots reduce them, ties to the smaller k at every step.
//   refit   thread t adds the 23 distinct float64 sums of the normal equations over its inlier rows t, t + 256, ... in order; six
//           butterfly steps (v = v + the partner's v: the same bits in every lane) and ((w0 + w1) + w2) + w3 over the waves; every
//           thread then runs the same unrolled 8 x 8 Cholesky in registers, so nothing has to be broadcast.
//   mask    the score's test again under the final model.
// No atomics, no allocation, no host copy, nothing read back, no workspace: one launch on the caller's stream, capturable in a graph.
#include <climits>
#include <cmath>
#include <initializer_list>

#include "common.h"
#include "prof.h"

namespace {

constexpr int kThreads = 256, kWave = 64, kWaves = kThreads / kWave;
constexpr int kMaxRows = 1024, kMaxDraws = 16, kSums = 23, kMaxHyp = 65536;

__device__ __forceinline__ uint32_t hf_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

__device__ __forceinline__ float hf_dot3(float a, float x, float b, float y, float c) {       // (a*x + b*y) + c
    return __fadd_rn(__fadd_rn(__fmul_rn(a, x), __fmul_rn(b, y)), c);
}

__device__ __forceinline__ bool hf_inlier(const float (&h)[8], float4 r, float hw, float hh, float thr2, float w_min) {
    const float u = hf_dot3(h[0], r.x, h[1], r.y, h[2]), v = hf_dot3(h[3], r.x, h[4], r.y, h[5]), w = hf_dot3(h[6], r.x, h[7], r.y, 1.0f);
    const float ex = __fmul_rn(__fsub_rn(__fdiv_rn(u, w), r.z), hw), ey = __fmul_rn(__fsub_rn(__fdiv_rn(v, w), r.w), hh);
    return w > w_min && __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)) <= thr2;                 // (false for NaN)
}

// adj of [[x0, x1, x2], [y0, y1, y2], [1, 1, 1]], row i = a[i][0..2], and l[i] = (a[i][0]*x3 + a[i][1]*y3) + a[i][2]
__device__ __forceinline__ void hf_basis(float x0, float y0, float x1, float y1, float x2, float y2, float x3, float y3, float (&a)[3][3],
                                         float (&l)[3]) {
    a[0][0] = __fsub_rn(y1, y2); a[0][1] = __fsub_rn(x2, x1); a[0][2] = __fsub_rn(__fmul_rn(x1, y2), __fmul_rn(x2, y1));
    a[1][0] = __fsub_rn(y2, y0); a[1][1] = __fsub_rn(x0, x2); a[1][2] = __fsub_rn(__fmul_rn(x2, y0), __fmul_rn(x0, y2));
    a[2][0] = __fsub_rn(y0, y1); a[2][1] = __fsub_rn(x1, x0); a[2][2] = __fsub_rn(__fmul_rn(x0, y1), __fmul_rn(x1, y0));
#pragma unroll
    for (int i = 0; i < 3; ++i) l[i] = hf_dot3(a[i][0], x3, a[i][1], y3, a[i][2]);
}

// H = [q0 q1 q2] diag(s) adj([p0 p1 p2]), s_i = mu_i * (lambda_j * lambda_k); h = H / H[8].  -> every entry finite
__device__ __forceinline__ bool hf_four_point(float4 r0, float4 r1, float4 r2, float4 r3, float (&h)[8]) {
    float a[3][3], b[3][3], l[3], m[3];
    hf_basis(r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, r3.x, r3.y, a, l);
    hf_basis(r0.z, r0.w, r1.z, r1.w, r2.z, r2.w, r3.z, r3.w, b, m);
    const float s[3] = {__fmul_rn(m[0], __fmul_rn(l[1], l[2])), __fmul_rn(m[1], __fmul_rn(l[0], l[2])), __fmul_rn(m[2], __fmul_rn(l[0], l[1]))};
    const float t[3][3] = {{__fmul_rn(r0.z, s[0]), __fmul_rn(r1.z, s[1]), __fmul_rn(r2.z, s[2])},
                           {__fmul_rn(r0.w, s[0]), __fmul_rn(r1.w, s[1]), __fmul_rn(r2.w, s[2])},
                           {s[0], s[1], s[2]}};
    float g[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            g[3 * r + c] = __fadd_rn(__fadd_rn(__fmul_rn(t[r][0], a[0][c]), __fmul_rn(t[r][1], a[1][c])), __fmul_rn(t[r][2], a[2][c]));
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        h[i] = __fdiv_rn(g[i], g[8]);
        ok = ok && fabsf(h[i]) < INFINITY;                                          // (false for NaN)
    }
    return ok;
}

__global__ __launch_bounds__(kThreads) void homfit_kernel(const float4* __restrict__ rows, const int* __restrict__ nrows, int M, float hw, float hh,
                                                          int hyp, float thr2, int need, uint32_t seed, float w_min, float* __restrict__ Hm,
                                                          unsigned char* __restrict__ mask, int* __restrict__ count, int* __restrict__ status,
                                                          int* __restrict__ best) {
    __shared__ float4 sRow[kMaxRows];
    __shared__ double sSum[kWaves][kSums];
    __shared__ float sH[8];
    __shared__ int sC[kWaves], sK[kWaves], sCnt[kWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave, pair = blockIdx.x;
    int n = nrows[pair];
    n = n < 0 ? 0 : (n > M ? M : n);                                                // nothing past row n (or M) is read
    for (int i = tid; i < n; i += kThreads) sRow[i] = rows[(size_t)pair * M + i];
    __syncthreads();

    // ---- hypotheses: sample, four-point model, score ----
    int myc = -1, myk = INT_MAX;
    float myh[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (n >= 4) {
        const uint32_t chain = hf_mix(hf_mix(seed + 0x9e3779b9u) + (uint32_t)pair);
        for (int k = tid; k < hyp; k += kThreads) {
            const uint32_t base = hf_mix(chain + (uint32_t)k);
            int i0 = -1, i1 = -1, i2 = -1, i3 = -1, got = 0;
#pragma unroll
            for (int d = 0; d < kMaxDraws; ++d) {
                const int j = (int)(((unsigned long long)hf_mix(base + (uint32_t)d) * (unsigned long long)(uint32_t)n) >> 32);
                const bool take = got < 4 && j != i0 && j != i1 && j != i2 && j != i3;
                i0 = take && got == 0 ? j : i0;
                i1 = take && got == 1 ? j : i1;
                i2 = take && got == 2 ? j : i2;
                i3 = take && got == 3 ? j : i3;
                got += take ? 1 : 0;
            }
            int c = -1;
            float h[8];
            if (got == 4 && hf_four_point(sRow[i0], sRow[i1], sRow[i2], sRow[i3], h)) {
                c = 0;
                for (int i = 0; i < n; ++i) c += hf_inlier(h, sRow[i], hw, hh, thr2, w_min) ? 1 : 0;
            }
            if (c > myc) {                                                          // k grows: a tie keeps the smaller k
                myc = c; myk = k;
#pragma unroll
                for (int i = 0; i < 8; ++i) myh[i] = h[i];
            }
        }
    }
    int bc = myc, bk = myk;
#pragma unroll
    for (int d = kWave / 2; d; d >>= 1) {
        const int oc = __shfl_xor(bc, d), ok = __shfl_xor(bk, d);
        if (oc > bc || (oc == bc && ok < bk)) { bc = oc; bk = ok; }
    }
    if (lane == 0) { sC[wave] = bc; sK[wave] = bk; }
    __syncthreads();
    bc = sC[0]; bk = sK[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w)
        if (sC[w] > bc || (sC[w] == bc && sK[w] < bk)) { bc = sC[w]; bk = sK[w]; }
    if (n < 4 || bc < need) {                                                       // (uniform) no model
        for (int i = tid; i < M; i += kThreads) mask[(size_t)pair * M + i] = 0;
        if (tid < 9) Hm[(size_t)pair * 9 + tid] = 0.0f;
        if (tid == 0) { count[pair] = 0; status[pair] = 0; best[pair] = -1; }
        return;
    }
    if (myk == bk) {                                                                // one thread: k is unique
#pragma unroll
        for (int i = 0; i < 8; ++i) sH[i] = myh[i];
    }
    __syncthreads();
    float hb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) hb[i] = sH[i];

    // ---- refit: the 23 distinct sums of the normal equations of the DLT with h33 = 1, in float64 ----
    double S[kSums];
#pragma unroll
    for (int j = 0; j < kSums; ++j) S[j] = 0.0;
    for (int i = tid; i < n; i += kThreads) {
        const float4 r = sRow[i];
        if (!hf_inlier(hb, r, hw, hh, thr2, w_min)) continue;
        const double x = r.x, y = r.y, u = r.z, v = r.w;
        const double xx = __dmul_rn(x, x), xy = __dmul_rn(x, y), yy = __dmul_rn(y, y), q = __dadd_rn(__dmul_rn(u, u), __dmul_rn(v, v));
        const double ux = __dmul_rn(u, x), uy = __dmul_rn(u, y), vx = __dmul_rn(v, x), vy = __dmul_rn(v, y);
        const double term[kSums] = {xx, xy, x, yy, y, 1.0,
                                    __dmul_rn(ux, x), __dmul_rn(ux, y), ux, __dmul_rn(uy, y), uy, u,
                                    __dmul_rn(vx, x), __dmul_rn(vx, y), vx, __dmul_rn(vy, y), vy, v,
                                    __dmul_rn(q, xx), __dmul_rn(q, xy), __dmul_rn(q, yy), __dmul_rn(q, x), __dmul_rn(q, y)};
#pragma unroll
        for (int j = 0; j < kSums; ++j) S[j] = __dadd_rn(S[j], term[j]);
    }
#pragma unroll
    for (int j = 0; j < kSums; ++j) {
#pragma unroll
        for (int d = kWave / 2; d; d >>= 1) S[j] = __dadd_rn(S[j], __shfl_xor(S[j], d));
        if (lane == 0) sSum[wave][j] = S[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSums; ++j) S[j] = __dadd_rn(__dadd_rn(__dadd_rn(sSum[0][j], sSum[1][j]), sSum[2][j]), sSum[3][j]);

    // unknowns h0..h7; the rows (x, y, 1, 0, 0, 0, -ux, -uy | u) and (0, 0, 0, x, y, 1, -vx, -vy | v); lower triangle of A^T A, A^T b
    double L[8][8], rhs[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) L[i][j] = 0.0;
    L[0][0] = S[0]; L[1][0] = S[1]; L[1][1] = S[3]; L[2][0] = S[2]; L[2][1] = S[4]; L[2][2] = S[5];
    L[3][3] = S[0]; L[4][3] = S[1]; L[4][4] = S[3]; L[5][3] = S[2]; L[5][4] = S[4]; L[5][5] = S[5];
    L[6][0] = -S[6]; L[6][1] = -S[7]; L[6][2] = -S[8]; L[6][3] = -S[12]; L[6][4] = -S[13]; L[6][5] = -S[14]; L[6][6] = S[18];
    L[7][0] = -S[7]; L[7][1] = -S[9]; L[7][2] = -S[10]; L[7][3] = -S[13]; L[7][4] = -S[15]; L[7][5] = -S[16]; L[7][6] = S[19]; L[7][7] = S[20];
    rhs[0] = S[8]; rhs[1] = S[10]; rhs[2] = S[11]; rhs[3] = S[14]; rhs[4] = S[16]; rhs[5] = S[17]; rhs[6] = -S[21]; rhs[7] = -S[22];
    bool good = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) {                                                   // Cholesky, column by column, in place
        double d = L[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d = __dsub_rn(d, __dmul_rn(L[j][k], L[j][k]));
        good = good && d > 0.0;                                                     // (false for NaN; the arithmetic goes on)
        L[j][j] = __dsqrt_rn(d);
#pragma unroll
        for (int i = j + 1; i < 8; ++i) {
            double s = L[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = __dsub_rn(s, __dmul_rn(L[i][k], L[j][k]));
            L[i][j] = __ddiv_rn(s, L[j][j]);
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {                                                   // L z = rhs
        double s = rhs[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = __dsub_rn(s, __dmul_rn(L[i][k], rhs[k]));
        rhs[i] = __ddiv_rn(s, L[i][i]);
    }
#pragma unroll
    for (int i = 7; i >= 0; --i) {                                                  // L^T h = z
        double s = rhs[i];
#pragma unroll
        for (int k = i + 1; k < 8; ++k) s = __dsub_rn(s, __dmul_rn(L[k][i], rhs[k]));
        rhs[i] = __ddiv_rn(s, L[i][i]);
    }
    float hf[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        hf[i] = __double2float_rn(rhs[i]);
        good = good && fabsf(hf[i]) < INFINITY;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) hf[i] = good ? hf[i] : hb[i];

    // ---- the final mask and count ----
    int c = 0;
    for (int i = tid; i < M; i += kThreads) {
        const bool in = i < n && hf_inlier(hf, sRow[i < n ? i : 0], hw, hh, thr2, w_min);
        mask[(size_t)pair * M + i] = in ? 1 : 0;
        c += in ? 1 : 0;
    }
#pragma unroll
    for (int d = kWave / 2; d; d >>= 1) c += __shfl_xor(c, d);
    if (lane == 0) sCnt[wave] = c;
    __syncthreads();
    if (tid == 0) {
        float* o = Hm + (size_t)pair * 9;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = hf[i];
        o[8] = 1.0f;
        count[pair] = sCnt[0] + sCnt[1] + sCnt[2] + sCnt[3];
        status[pair] = good ? 1 : 2;
        best[pair] = bk;
    }
}

}  // namespace

extern "C" {

/* See include/stabnet_hip.h. */
int stabnet_homfit(const float* matches, const int* n, int B, int M, int H, int W, int hypotheses, float thr_px, int min_inliers, int seed,
                   float w_min, float* Hm, unsigned char* mask, int* count, int* status, int* best, void* stream, void* profp) {
    SN_REQUIRE(matches && n && Hm && mask && count && status && best, "homfit: null pointer");
    SN_REQUIRE(B >= 1 && B <= 65535, "homfit: B must be 1..65535, got %d", B);
    SN_REQUIRE(M >= 4 && M <= kMaxRows, "homfit: M must be 4..%d (a pair's rows are staged in 16 KiB of LDS), got %d", kMaxRows, M);
    SN_REQUIRE(H >= 1 && H <= 1 << 20 && W >= 1 && W <= 1 << 20, "homfit: H and W must be 1..2^20, got %d x %d", H, W);
    SN_REQUIRE(hypotheses >= 1 && hypotheses <= kMaxHyp, "homfit: hypotheses must be 1..%d, got %d", kMaxHyp, hypotheses);
    SN_REQUIRE(thr_px > 0.0f && thr_px < INFINITY, "homfit: thr_px must be positive and finite, got %g", thr_px);
    SN_REQUIRE(min_inliers >= 0, "homfit: min_inliers must not be negative, got %d", min_inliers);
    SN_REQUIRE(seed >= 0, "homfit: seed must be 0..2^31 - 1, got %d", seed);
    SN_REQUIRE(w_min >= 0.0f && w_min < INFINITY, "homfit: w_min must be finite and not negative, got %g", w_min);
    SN_REQUIRE(((uintptr_t)matches & 15) == 0, "homfit: matches must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    for (const void* p : {(const void*)matches, (const void*)n, (const void*)Hm, (const void*)mask, (const void*)count, (const void*)status,
                          (const void*)best}) {
        const int rc = sn_check_device(p, "homfit: a pointer", st);
        if (rc) return rc;
    }
    Prof* prof = static_cast<Prof*>(profp);
    const bool rec = prof && prof->begin(st);
    homfit_kernel<<<dim3(B), kThreads, 0, st>>>(reinterpret_cast<const float4*>(matches), n, M, 0.5f * (float)W, 0.5f * (float)H, hypotheses,
                                                thr_px * thr_px, min_inliers > 4 ? min_inliers : 4, (uint32_t)seed, w_min, Hm, mask, count,
                                                status, best);
    if (rec) prof->end(st, PK_KERNEL_HOMFIT, 0.0, (double)B * (17.0 * M + 52.0), hypotheses);  // the rows once, the mask, the small outputs
    SN_LAUNCH_CHECK("homfit_kernel");
    return STABNET_OK;
}

}  // extern "C"
