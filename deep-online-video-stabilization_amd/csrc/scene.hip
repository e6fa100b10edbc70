// Scene cuts of the online loop (include/stabnet_hip.h, "scene cuts"): an all-integer statistic of the incoming grey frame -- 32-bin
// histograms of a 4 x 4 grid of tiles -- compared with the previous frame's ON THE DEVICE, a flag in device memory, and a ring reseed
// predicated on that flag.  Everything has fixed arguments and nothing reads back: the three launches sit in the frame's hipGraph.
// Integer counters only: any grid shape and any order of the atomics gives the same bits.
#include "common.h"

#define SCENE_TILES 16
#define SCENE_BINS 32
#define SCENE_HIST (SCENE_TILES * SCENE_BINS)                 // 512 counters per histogram
#define SCENE_WORDS (2 + 2 * SCENE_HIST)                      // {seen, since, prev[16][32], cur[16][32]}
#define SCENE_THREADS 256
#define SCENE_PIX_PER_WG 2048                                 // 8 pixels per thread: a 288 x 512 frame is 72 workgroups
#define SCENE_COPIES 32                                       // private LDS histograms: 4 waves x 8 lane groups

// bin of one train-normalised grey value: every operation one float32 rounding (the build has -ffp-contract=off); a NaN lands in 0
__device__ __forceinline__ int scene_bin(float g) {
    float t = floorf((g + 0.5f) * 255.0f + 0.5f);
    t = fminf(fmaxf(t, 0.f), 255.f);
    return (int)t >> 3;
}

// tile column of pixel x: 4*x / W by the three column bounds b[k] = ceil(k*W / 4)  (4x >= kW  <=>  x >= ceil(kW / 4))
__device__ __forceinline__ int scene_tx(int x, int b1, int b2, int b3) { return (x >= b1) + (x >= b2) + (x >= b3); }

// One workgroup = up to SCENE_PIX_PER_WG consecutive pixels of ONE tile row (rows [ceil(ty*H/4), ceil((ty+1)*H/4)) are contiguous in
// memory).  Counters: 4 tile columns x 32 bins, one private copy per (wave, lane & 7) so that a flat image puts 8 lanes, not 64, on
// one LDS address; copy c of counter i lies at i*32 + c: the copies of one counter are 32 consecutive banks.  Then one integer atomicAdd
// per non-zero counter into the stream's zeroed `cur`.
template <bool VEC4>
__global__ __launch_bounds__(SCENE_THREADS) void scene_hist_kernel(const float* __restrict__ grey, int H, int W,
                                                                  unsigned* __restrict__ state) {
    __shared__ unsigned lds[4 * SCENE_BINS * SCENE_COPIES];
    const int ty = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
    for (int i = tid; i < 4 * SCENE_BINS * SCENE_COPIES; i += SCENE_THREADS) lds[i] = 0u;
    __syncthreads();
    const int r0 = (ty * H + 3) >> 2, r1 = ((ty + 1) * H + 3) >> 2;
    const int p0 = r0 * W, p1 = r1 * W;                       // this tile row's pixels of the image (H*W < 2^30)
    const int a = p0 + (int)blockIdx.x * SCENE_PIX_PER_WG;
    const int e = (a + SCENE_PIX_PER_WG < p1) ? a + SCENE_PIX_PER_WG : p1;
    const int b1 = (W + 3) >> 2, b2 = (2 * W + 3) >> 2, b3 = (3 * W + 3) >> 2;
    const int copy = ((tid >> 6) << 3) | (tid & 7);
    const float* img = grey + (long)n * H * W;
    if (VEC4) {                                               // W % 4 == 0, 16-byte aligned: four pixels of one row per load
        for (int p = a + 4 * tid; p < e; p += 4 * SCENE_THREADS) {
            const float4 v = *reinterpret_cast<const float4*>(img + p);
            const int x = (int)((unsigned)p % (unsigned)W);
            atomicAdd(&lds[((scene_tx(x, b1, b2, b3) << 5) + scene_bin(v.x)) * SCENE_COPIES + copy], 1u);
            atomicAdd(&lds[((scene_tx(x + 1, b1, b2, b3) << 5) + scene_bin(v.y)) * SCENE_COPIES + copy], 1u);
            atomicAdd(&lds[((scene_tx(x + 2, b1, b2, b3) << 5) + scene_bin(v.z)) * SCENE_COPIES + copy], 1u);
            atomicAdd(&lds[((scene_tx(x + 3, b1, b2, b3) << 5) + scene_bin(v.w)) * SCENE_COPIES + copy], 1u);
        }
    } else {
        for (int p = a + tid; p < e; p += SCENE_THREADS) {
            const int x = (int)((unsigned)p % (unsigned)W);
            atomicAdd(&lds[((scene_tx(x, b1, b2, b3) << 5) + scene_bin(img[p])) * SCENE_COPIES + copy], 1u);
        }
    }
    __syncthreads();
    if (tid < 4 * SCENE_BINS) {                               // counter tid = tx*32 + bin; rotated start: two lanes per bank, not 32
        unsigned s = 0u;
#pragma unroll 8
        for (int c = 0; c < SCENE_COPIES; ++c) s += lds[tid * SCENE_COPIES + ((c + tid) & (SCENE_COPIES - 1))];
        if (s != 0u) atomicAdd(&state[(long)n * SCENE_WORDS + 2 + SCENE_HIST + ty * 4 * SCENE_BINS + tid], s);
    }
}

// One workgroup per stream, one thread per counter: D = sum |cur - prev|, the rule, then prev = cur and cur = 0 for the next call.
__global__ __launch_bounds__(SCENE_HIST) void scene_decide_kernel(unsigned* __restrict__ state, unsigned thr_num, unsigned min_gap,
                                                                  int* __restrict__ flag, unsigned* __restrict__ dist) {
    __shared__ unsigned part[SCENE_HIST / 64];
    const int n = blockIdx.x, tid = threadIdx.x;
    unsigned* st = state + (long)n * SCENE_WORDS;
    const unsigned c = st[2 + SCENE_HIST + tid], p = st[2 + tid];
    unsigned d = c > p ? c - p : p - c;                       // D <= 2*H*W < 2^32 for H, W <= 32767
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_down(d, o, 64);
    if ((tid & 63) == 0) part[tid >> 6] = d;
    st[2 + tid] = c;
    st[2 + SCENE_HIST + tid] = 0u;
    __syncthreads();
    if (tid == 0) {
        unsigned D = 0u;
#pragma unroll
        for (int w = 0; w < SCENE_HIST / 64; ++w) D += part[w];
        const unsigned seen = st[0], since = st[1];
        int f = 0;
        if (seen == 0u) D = 0u;
        else f = (since >= min_gap && D > thr_num) ? 1 : 0;
        st[1] = f ? 0u : (since == 0xffffffffu ? since : since + 1u);
        st[0] = seen == 0xffffffffu ? seen : seen + 1u;
        flag[n] = f;
        dist[n] = D;
    }
}

// stabnet_ring_init for the streams whose flag is set; a workgroup of another stream loads the flag and returns.
__global__ __launch_bounds__(256) void ring_reseed_if_kernel(float* __restrict__ frames, float* __restrict__ masks,
                                                             const float* __restrict__ first, int depth, long hw,
                                                             const int* __restrict__ flag) {
    const int s = blockIdx.y;
    if (flag[s] == 0) return;
    const long i0 = (long)blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long i = i0 + 256 * k;
        if (i >= hw) break;
        const float v = first[(long)s * hw + i];
        for (int d = 0; d < depth; ++d) {
            frames[((long)s * depth + d) * hw + i] = v;
            masks[((long)s * depth + d) * hw + i] = 0.f;
        }
    }
}

extern "C" {

int stabnet_scene_state_words(void) { return SCENE_WORDS; }

int stabnet_scene_update(const float* grey, int N, int H, int W, unsigned thr_num, int min_gap, unsigned* state, int* flag,
                         unsigned* dist, void* stream) {
    SN_REQUIRE(grey && state && flag && dist, "scene_update: null pointer");
    SN_REQUIRE(N >= 1 && N <= 65535, "scene_update: batch %d outside 1..65535", N);
    SN_REQUIRE(H >= 4 && H <= 32767 && W >= 4 && W <= 32767, "scene_update: frame %dx%d outside 4..32767 (a 4 x 4 grid of tiles, 32-bit counts)", H, W);
    SN_REQUIRE(min_gap >= 0, "scene_update: min_gap %d is negative", min_gap);
    hipStream_t st = (hipStream_t)stream;
    int rc = sn_check_device(grey, "scene_update: grey", st);
    if (rc == 0) rc = sn_check_device(state, "scene_update: state", st);
    if (rc == 0) rc = sn_check_device(flag, "scene_update: flag", st);
    if (rc == 0) rc = sn_check_device(dist, "scene_update: dist", st);
    if (rc) return rc;
    // the tallest tile row has ceil(H / 4) rows
    const long row_pix = (long)((H + 3) >> 2) * W;
    const dim3 grid(cdiv(row_pix, SCENE_PIX_PER_WG), 4, N);
    if (W % 4 == 0 && ((size_t)grey & 15) == 0)
        scene_hist_kernel<true><<<grid, SCENE_THREADS, 0, st>>>(grey, H, W, state);
    else
        scene_hist_kernel<false><<<grid, SCENE_THREADS, 0, st>>>(grey, H, W, state);
    SN_LAUNCH_CHECK("scene_hist_kernel");
    scene_decide_kernel<<<N, SCENE_HIST, 0, st>>>(state, thr_num, (unsigned)min_gap, flag, dist);
    SN_LAUNCH_CHECK("scene_decide_kernel");
    return STABNET_OK;
}

int stabnet_ring_reseed_if(float* frames_ring, float* masks_ring, const float* first_frame, int S, int depth, int H, int W,
                           const int* flag, void* stream) {
    SN_REQUIRE(frames_ring && masks_ring && first_frame && S > 0 && S <= 65535 && depth > 0 && H > 0 && W > 0,
               "ring_reseed_if: bad arguments");
    SN_REQUIRE(flag != nullptr, "ring_reseed_if: null flag (an unconditional reseed is stabnet_ring_init)");
    hipStream_t st = (hipStream_t)stream;
    int rc = sn_check_device(frames_ring, "ring_reseed_if: frames_ring", st);
    if (rc == 0) rc = sn_check_device(masks_ring, "ring_reseed_if: masks_ring", st);
    if (rc == 0) rc = sn_check_device(first_frame, "ring_reseed_if: first_frame", st);
    if (rc == 0) rc = sn_check_device(flag, "ring_reseed_if: flag", st);
    if (rc) return rc;
    const long hw = (long)H * W;
    ring_reseed_if_kernel<<<dim3(cdiv(hw, 1024), S), 256, 0, st>>>(frames_ring, masks_ring, first_frame, depth, hw, flag);
    SN_LAUNCH_CHECK("ring_reseed_if_kernel");
    return STABNET_OK;
}

}  // extern "C"
