// Second entropy back end of the JPEG decoder, gfx950: a stream WITHOUT restart markers (one interval: what OpenCV, ffmpeg and
// cameras write) decoded on the device from its uploaded bytes by self-synchronising parallel Huffman decoding (jpeg_sync.h: states,
// the walk, why an accepted chain is the sequential decode).  One lane per chunk of `chunk` bytes.  Per call, on the caller's stream,
// without host synchronisation, allocation or copy and with a launch count fixed at enqueue time (capturable in a hipGraph):
//   memset                  status words
//   mjpegd_sync_kernel<0>   guess: zero-fill the coefficients; every lane walks its chunk from a guessed state; then up to `rounds`
//                           rounds inside the workgroup: a lane whose entry is not its left neighbour's exit takes it and walks again
//   mjpegd_sync_kernel<1>   the same rounds once more, the first lane of every workgroup entering from the exit the workgroup in front
//                           recorded (not launched with rounds = 0)
//   mjpegd_sync_repair      one workgroup per frame: finds every chunk whose entry is not the exit in front of it, left to right, and
//                           one lane walks it again (slow, bounded, always right; one pass over the states when nothing is left);
//                           then the exclusive scan of (blocks started, DC differences per component) over the chunks
//   mjpegd_sync_kernel<2>   write: every lane walks its chunk from its accepted entry and stores the coefficients of its blocks, in
//                           natural order, DC as (short)(predictor + difference) from the scanned sums
// and the IDCT and colour launches of mjpeg_decode.hip.  A workgroup stages the bytes of its chunks (dword loads) and the four Huffman
// tables in LDS; the walks read nothing else.  stabnet_mjpeg_decode_sync_i420: the same launches in front of the IDCT and the crop to the
// dense I420 frame (mjpeg_decode.hip: mjpegd_launch_i420), the status words zeroed by a launch instead of the memset.
#include "common.h"
#include "jpeg_sync.h"
#include "jpeg_tables.h"
#include "mjpeg_decode.h"

namespace {

__constant__ const unsigned char d_zigzag_sync[64] = JPEG_ZIGZAG_INIT;

constexpr int kSyncLdsBytes = 32768;          // chunk bytes a workgroup stages: 256 chunks of up to 128 bytes, fewer of longer ones
constexpr int kSyncPad = 64;                  // behind them: the last symbol of a chunk (<= 8 stream bytes) and what fill() reads ahead

struct JsWs {                                 // the part of a frame's workspace behind the decoder's own
    JsState* entry;
    JsState* exits;
    JsSum* sums;                              // per chunk; after the scan: exclusive prefix
    JsState* group_exit;                      // per workgroup of the guess launch: the exit of its last chunk
};

inline size_t js_ws_bytes(int nc_max, int ngroups) { return jd_align16((size_t)nc_max * (2 * sizeof(JsState) + sizeof(JsSum)) + (size_t)ngroups * sizeof(JsState)); }

__host__ __device__ inline JsWs js_ws(unsigned char* base, int nc_max) {
    JsWs w;
    w.sums = reinterpret_cast<JsSum*>(base);                                          // 16-byte elements first
    w.entry = reinterpret_cast<JsState*>(base + (size_t)nc_max * sizeof(JsSum));
    w.exits = w.entry + nc_max;
    w.group_exit = w.exits + nc_max;
    return w;
}

struct JsFrame { bool ok; int a, b, nc; };

// Every offset of the blob is checked against the launch's geometry and the slot's size before it is used.
template <int MODE>
__device__ __forceinline__ JsFrame js_frame(const unsigned char* slot, size_t in_stride, int H, int W, int nmcu, size_t blob_max, int chunk,
                                            int nc_max) {
    const JdBlobHead* hd = reinterpret_cast<const JdBlobHead*>(slot);
    const int nbytes = hd->nbytes;
    JsFrame f;
    f.ok = hd->magic == kJdMagic && hd->H == H && hd->W == W && hd->mode == MODE && hd->nmcu == nmcu && hd->restart_mcus == nmcu &&
           hd->nint == 1 && nbytes >= 0 && blob_max + (size_t)nbytes <= in_stride && kJdBlobStarts + 2 * sizeof(int) <= blob_max;
#pragma unroll
    for (int c = 0; c < 3; ++c) f.ok = f.ok && (unsigned)hd->td[c] <= 1u && (unsigned)hd->ta[c] <= 1u;
    const int* starts = reinterpret_cast<const int*>(slot + kJdBlobStarts);
    f.a = starts[0]; f.b = starts[1] - 2;
    f.ok = f.ok && f.a >= 0 && f.a <= f.b && f.b <= nbytes;
    f.nc = f.ok ? js_nchunks(f.a, f.b, chunk) : 0;
    f.ok = f.ok && f.nc <= nc_max;
    return f;
}

__device__ __forceinline__ void js_stage_tables(const unsigned char* slot, JdHuff* s_huff, int* s_sel, unsigned char* s_zz) {
    const JdBlobHead* hd = reinterpret_cast<const JdBlobHead*>(slot);
    const unsigned* src = reinterpret_cast<const unsigned*>(slot + kJdBlobHuff);
    unsigned* dst = reinterpret_cast<unsigned*>(s_huff);
    for (int i = threadIdx.x; i < (int)(4 * sizeof(JdHuff) / 4); i += 256) dst[i] = src[i];
    if (threadIdx.x < 64) s_zz[threadIdx.x] = d_zigzag_sync[threadIdx.x];
    if (threadIdx.x < 3) { s_sel[threadIdx.x] = hd->td[threadIdx.x]; s_sel[3 + threadIdx.x] = hd->ta[threadIdx.x]; }
}

// Stream bytes [lo, hi) -> s_data, as the dwords that hold them (the stream starts 16-byte aligned inside a slot whose size is a
// multiple of 16, so the dwords lie inside the slot).  -> the pointer p with p[i] = stream byte i for lo <= i < hi.
__device__ __forceinline__ const unsigned char* js_stage_bytes(const unsigned char* stream, int lo, int hi, unsigned* s_data, int cap_dwords) {
    const int lo4 = lo & ~3;
    int nd = hi > lo4 ? (hi - lo4 + 3) >> 2 : 0;
    nd = min(nd, cap_dwords);
    const unsigned* src = reinterpret_cast<const unsigned*>(stream + lo4);
    for (int i = threadIdx.x; i < nd; i += 256) s_data[i] = src[i];
    return reinterpret_cast<const unsigned char*>(s_data) - lo4;
}

// PHASE 0 guess (+ rounds), 1 hand-over across workgroups (+ rounds), 2 write.  Workgroup w of frame blockIdx.y owns the chunks
// [w cpw, (w + 1) cpw), lane l the chunk w cpw + l.  Dynamic LDS: cpw * chunk + kSyncPad bytes.
template <int MODE, int PHASE>
__global__ __launch_bounds__(256) void mjpegd_sync_kernel(const unsigned char* __restrict__ in, size_t in_stride, int H, int W, int nmcu,
                                                          size_t blob_max, int chunk, int cpw, int rounds, short* __restrict__ coef,
                                                          size_t coef_frame_stride, int* __restrict__ status, unsigned char* sync,
                                                          size_t sync_frame, int nc_max) {
    constexpr int BPM = MODE == JD_MODE_420 ? 6 : (MODE == JD_MODE_444 ? 3 : 1);
    extern __shared__ __attribute__((aligned(16))) unsigned s_data[];
    __shared__ __attribute__((aligned(16))) JdHuff s_huff[4];
    __shared__ unsigned char s_zz[64];
    __shared__ int s_sel[6];
    __shared__ JsState s_exit[2][256];
    const int n = blockIdx.y, wg = blockIdx.x, l = threadIdx.x;
    const unsigned char* slot = in + (size_t)n * in_stride;
    const JsFrame f = js_frame<MODE>(slot, in_stride, H, W, nmcu, blob_max, chunk, nc_max);
    const long nblk = (long)nmcu * BPM;
    short* cf = coef + (size_t)n * coef_frame_stride;
    if (PHASE == 0) {                        // zero the coefficients, whatever the blob says
        uint4* z = reinterpret_cast<uint4*>(cf);
        for (long i = (long)wg * 256 + l; i < nblk * 8; i += (long)gridDim.x * 256) z[i] = make_uint4(0u, 0u, 0u, 0u);
        if (!f.ok && wg == 0 && l == 0) atomicOr(status + n, JD_ERR_BLOB);
    }
    if (!f.ok || (long)wg * cpw >= f.nc) return;
    const JsWs ws = js_ws(sync + (size_t)n * sync_frame, nc_max);
    js_stage_tables(slot, s_huff, s_sel, s_zz);
    const long w0 = (long)f.a + (long)wg * cpw * chunk;                  // < b, as the workgroup has a chunk
    const int lo = (int)max((long)f.a, w0 - 1);                           // the guess looks one byte back
    const int hi = (int)min((long)f.b, w0 + (long)cpw * chunk + kSyncPad - 8);
    const unsigned char* data = js_stage_bytes(slot + blob_max, lo, hi, s_data, (cpw * chunk + kSyncPad) >> 2);
    __syncthreads();
    const int c = wg * cpw + l;
    const bool active = l < cpw && c < f.nc;
    const int limit = active ? js_limit(c, f.nc, f.a, chunk) : 0;
    JsState entry, ex;
    JsSum sm;
    entry.pos = 0; entry.meta = JS_DEAD; ex = entry;
    sm.cnt = sm.dc0 = sm.dc1 = sm.dc2 = 0u;
    if (PHASE == 2) {
        if (!active) return;
        const JsSum at = ws.sums[c];
        const int err = js_walk<true>(data, hi, limit, ws.entry[c], s_huff, s_sel, s_sel + 3, MODE, &ex, &sm, (long)at.cnt - 1, nblk, at.dc0,
                                      at.dc1, at.dc2, cf, s_zz);
        if (err) atomicOr(status + n, err);
        return;
    }
    if (active) {
        if (PHASE == 0) {
            entry = js_guess(data, f.a, f.b, c, chunk);
            js_walk<false>(data, hi, limit, entry, s_huff, s_sel, s_sel + 3, MODE, &ex, &sm, 0, 0, 0u, 0u, 0u, nullptr, s_zz);
        } else {
            entry = ws.entry[c]; ex = ws.exits[c]; sm = ws.sums[c];
        }
    }
    JsState left;                            // PHASE 1, lane 0: what the workgroup in front left
    left.pos = 0; left.meta = 0;
    const bool handover = PHASE == 1 && l == 0 && wg > 0;
    if (handover) left = ws.group_exit[wg - 1];
    int cur = 0;
    s_exit[0][l] = ex;
    for (int r = 0; r < rounds; ++r) {
        __syncthreads();
        int changed = 0;
        if (active && (l > 0 || handover)) {
            const JsState x = l > 0 ? s_exit[cur][l - 1] : left;
            if (!js_same(x, entry)) {
                entry = x;
                js_walk<false>(data, hi, limit, entry, s_huff, s_sel, s_sel + 3, MODE, &ex, &sm, 0, 0, 0u, 0u, 0u, nullptr, s_zz);
                changed = 1;
            }
        }
        s_exit[cur ^ 1][l] = ex;
        cur ^= 1;
        if (!__syncthreads_or(changed)) break;
    }
    if (active) {
        ws.entry[c] = entry; ws.exits[c] = ex; ws.sums[c] = sm;
        if (PHASE == 0 && (l == cpw - 1 || c == f.nc - 1)) ws.group_exit[wg] = ex;
    }
}

// One workgroup per frame.  Dynamic LDS: chunk + kSyncPad bytes.
template <int MODE>
__global__ __launch_bounds__(256) void mjpegd_sync_repair_kernel(const unsigned char* __restrict__ in, size_t in_stride, int H, int W, int nmcu,
                                                                 size_t blob_max, int chunk, int* __restrict__ status,
                                                                 unsigned char* sync, size_t sync_frame, int nc_max,
                                                                 int* __restrict__ stats) {
    constexpr int BPM = MODE == JD_MODE_420 ? 6 : (MODE == JD_MODE_444 ? 3 : 1);
    extern __shared__ __attribute__((aligned(16))) unsigned s_data[];
    __shared__ __attribute__((aligned(16))) JdHuff s_huff[4];
    __shared__ unsigned char s_zz[64];
    __shared__ int s_sel[6];
    __shared__ int s_first;
    __shared__ JsSum s_part[2][256];
    const int n = blockIdx.x, l = threadIdx.x;
    const unsigned char* slot = in + (size_t)n * in_stride;
    const JsFrame f = js_frame<MODE>(slot, in_stride, H, W, nmcu, blob_max, chunk, nc_max);
    if (!f.ok) {
        if (stats && l < 2) stats[2 * n + l] = 0;
        return;
    }
    const JsWs ws = js_ws(sync + (size_t)n * sync_frame, nc_max);
    js_stage_tables(slot, s_huff, s_sel, s_zz);
    // 3. verify and repair: the first chunk at or behind `from` whose entry is not the exit in front of it, until there is none
    int from = 1, repaired = 0;
    for (;;) {
        int first = f.nc;
        for (int base = from; base < f.nc; base += 256) {
            __syncthreads();
            if (l == 0) s_first = f.nc;
            __syncthreads();
            const int c = base + l;
            if (c < f.nc && !js_same(ws.exits[c - 1], ws.entry[c])) atomicMin(&s_first, c);
            __syncthreads();
            first = s_first;
            if (first < f.nc) break;
        }
        if (first >= f.nc) break;
        const JsState x = ws.exits[first - 1];
        const int limit = js_limit(first, f.nc, f.a, chunk);
        const bool through = (x.meta & JS_DEAD) || x.pos >= limit;             // nothing of the chunk is read
        const int lo = through ? f.b : min(max(x.pos, f.a), f.b);
        const int hi = (int)min((long)f.b, (long)f.a + ((long)first + 1) * chunk + kSyncPad - 8);
        const unsigned char* data = js_stage_bytes(slot + blob_max, lo, hi, s_data, (chunk + kSyncPad) >> 2);
        __syncthreads();
        if (l == 0) {
            JsState ex;
            JsSum sm;
            js_walk<false>(data, hi, limit, x, s_huff, s_sel, s_sel + 3, MODE, &ex, &sm, 0, 0, 0u, 0u, 0u, nullptr, s_zz);
            ws.entry[first] = x; ws.exits[first] = ex; ws.sums[first] = sm;
        }
        __syncthreads();                     // the stores of lane 0 are the workgroup's from here on
        from = first + 1;
        ++repaired;
    }
    if (stats && l == 0) { stats[2 * n] = f.nc; stats[2 * n + 1] = f.nc - repaired; }
    // 4. exclusive scan over the chunks: lane l owns `per` consecutive ones
    const int per = (f.nc + 255) / 256;
    const int c0 = min(f.nc, l * per), c1 = min(f.nc, c0 + per);
    JsSum mine = {0u, 0u, 0u, 0u};
    for (int c = c0; c < c1; ++c) js_add(mine, ws.sums[c]);
    int cur = 0;
    s_part[0][l] = mine;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {      // inclusive, Hillis-Steele
        JsSum v = s_part[cur][l];
        if (l >= d) js_add(v, s_part[cur][l - d]);
        s_part[cur ^ 1][l] = v;
        cur ^= 1;
        __syncthreads();
    }
    JsSum run = {0u, 0u, 0u, 0u};
    if (l > 0) run = s_part[cur][l - 1];
    for (int c = c0; c < c1; ++c) {
        const JsSum t = ws.sums[c];
        ws.sums[c] = run;
        js_add(run, t);
    }
    if (l == 255 && (long)s_part[cur][255].cnt < (long)nmcu * BPM) atomicOr(status + n, JD_ERR_DATA);
}

template <int MODE>
int js_launch(const unsigned char* in, size_t in_stride, int N, int H, int W, const JdGeom& g, int chunk, int rounds, short* coef,
              size_t coef_stride, int* status, unsigned char* sync, size_t sync_frame, int nc_max, int cpw, int* stats, int stop,
              hipStream_t st) {
    const dim3 grid(cdiv(nc_max, cpw), N);
    const size_t lds = (size_t)cpw * chunk + kSyncPad;
    mjpegd_sync_kernel<MODE, 0><<<grid, 256, lds, st>>>(in, in_stride, H, W, g.nmcu, g.blob_max, chunk, cpw, rounds, coef, coef_stride, status,
                                                        sync, sync_frame, nc_max);
    SN_LAUNCH_CHECK("mjpegd_sync_kernel (guess)");
    if (stop == 1) return STABNET_OK;
    if (rounds > 0) {
        mjpegd_sync_kernel<MODE, 1><<<grid, 256, lds, st>>>(in, in_stride, H, W, g.nmcu, g.blob_max, chunk, cpw, rounds, coef, coef_stride,
                                                            status, sync, sync_frame, nc_max);
        SN_LAUNCH_CHECK("mjpegd_sync_kernel (hand-over)");
    }
    if (stop == 2) return STABNET_OK;
    mjpegd_sync_repair_kernel<MODE><<<N, 256, (size_t)chunk + kSyncPad, st>>>(in, in_stride, H, W, g.nmcu, g.blob_max, chunk, status, sync,
                                                                              sync_frame, nc_max, stats);
    SN_LAUNCH_CHECK("mjpegd_sync_repair_kernel");
    if (stop == 3) return STABNET_OK;
    mjpegd_sync_kernel<MODE, 2><<<grid, 256, lds, st>>>(in, in_stride, H, W, g.nmcu, g.blob_max, chunk, cpw, rounds, coef, coef_stride, status,
                                                        sync, sync_frame, nc_max);
    SN_LAUNCH_CHECK("mjpegd_sync_kernel (write)");
    return STABNET_OK;
}

// chunk_bytes as the caller gives it -> the value used, or 0 (refused)
int js_chunk(int chunk_bytes) {
    if (chunk_bytes == 0) return kJsDefaultChunk;
    return chunk_bytes >= 8 && chunk_bytes <= 4096 && (chunk_bytes & 3) == 0 ? chunk_bytes : 0;
}

struct JsPlan { int chunk, cpw, nc_max, ngroups; size_t frame; };

bool js_plan(const JdGeom& g, size_t in_stride, int chunk_bytes, JsPlan* p) {
    p->chunk = js_chunk(chunk_bytes);
    if (!p->chunk || in_stride < g.blob_max || in_stride - g.blob_max >= ((size_t)1 << 30)) return false;
    p->cpw = kSyncLdsBytes / p->chunk < 256 ? kSyncLdsBytes / p->chunk : 256;
    p->nc_max = (int)((in_stride - g.blob_max + p->chunk - 1) / p->chunk) + 1;
    p->ngroups = cdiv(p->nc_max, p->cpw);
    p->frame = js_ws_bytes(p->nc_max, p->ngroups);
    return true;
}

}  // namespace

extern "C" {

/* See include/stabnet_hip.h. */
size_t stabnet_mjpeg_decode_sync_workspace_bytes(int N, int H, int W, int C, int subsampling, size_t in_stride, int chunk_bytes) {
    JdGeom g;
    JsPlan p;
    if (N < 1 || !jd_geom(H, W, C, subsampling, &g) || !js_plan(g, in_stride, chunk_bytes, &p)) {
        stabnet_set_error("mjpeg_decode_sync_workspace_bytes: bad batch, shape, channels, subsampling, in_stride or chunk_bytes (0, or a "
                          "multiple of 4 in 8..4096)");
        return 0;
    }
    return (size_t)N * (g.frame + p.frame);
}

int stabnet_mjpeg_decode_sync(const unsigned char* in, size_t in_stride, int N, int H, int W, int C, int subsampling, unsigned char* out,
                              size_t row_stride, size_t frame_stride, int* status, void* workspace, size_t workspace_bytes, int stages,
                              int chunk_bytes, int rounds, int* stats, void* stream) {
    SN_REQUIRE(in && status && workspace, "mjpeg_decode_sync: null pointer");
    JdGeom g;
    SN_REQUIRE(N >= 1 && N <= 65535 && jd_geom(H, W, C, subsampling, &g), "mjpeg_decode_sync: bad batch, shape, channels (1 | 3) or subsampling (420 | 444)");
    SN_REQUIRE(stages >= -3 && stages <= 3 && stages != 0,
               "mjpeg_decode_sync: stages must be 1 (entropy), 2 (+ IDCT) or 3 (+ colour: the frame), or -1 .. -3 (stop inside the entropy decoding)");
    SN_REQUIRE(stages < 3 || out, "mjpeg_decode_sync: null pointer (out)");
    SN_REQUIRE(stages < 3 || (row_stride >= (size_t)W * C && (N == 1 || frame_stride >= (size_t)(H - 1) * row_stride + (size_t)W * C)),
               "mjpeg_decode_sync: row_stride %zu / frame_stride %zu too small for %dx%dx%d", row_stride, frame_stride, H, W, C);
    SN_REQUIRE(js_chunk(chunk_bytes), "mjpeg_decode_sync: chunk_bytes %d is not 0 (default) or a multiple of 4 in 8..4096", chunk_bytes);
    SN_REQUIRE(rounds >= -1 && rounds <= 1024, "mjpeg_decode_sync: rounds %d is not -1 (default) or 0..1024", rounds);
    SN_REQUIRE((in_stride & 15) == 0 && ((uintptr_t)in & 15) == 0, "mjpeg_decode_sync: in and in_stride must be 16-byte aligned");
    JsPlan p;
    SN_REQUIRE(in_stride >= g.blob_max && js_plan(g, in_stride, chunk_bytes, &p), "mjpeg_decode_sync: in_stride %zu < %zu (or 2^30 and above)",
               in_stride, g.blob_max);
    if (workspace_bytes < (size_t)N * (g.frame + p.frame)) {
        stabnet_set_error("mjpeg_decode_sync: workspace %zu < %zu bytes", workspace_bytes, (size_t)N * (g.frame + p.frame));
        return STABNET_ERR_WORKSPACE;
    }
    SN_REQUIRE(((uintptr_t)workspace & 15) == 0, "mjpeg_decode_sync: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int rc = sn_check_device(in, "mjpeg_decode_sync: in", st);
    if (rc == 0 && out) rc = sn_check_device(out, "mjpeg_decode_sync: out", st);
    if (rc == 0) rc = sn_check_device(workspace, "mjpeg_decode_sync: workspace", st);
    if (rc == 0) rc = sn_check_device(status, "mjpeg_decode_sync: status", st);
    if (rc == 0 && stats) rc = sn_check_device(stats, "mjpeg_decode_sync: stats", st);
    if (rc) return rc;
    unsigned char* wsb = static_cast<unsigned char*>(workspace);
    if (hipMemsetAsync(status, 0, (size_t)N * sizeof(int), st) != hipSuccess) {
        stabnet_set_error("mjpeg_decode_sync: hipMemsetAsync failed");
        return STABNET_ERR_LAUNCH;
    }
    short* coef = reinterpret_cast<short*>(wsb + g.coef);
    const size_t coef_stride = g.frame / sizeof(short);
    unsigned char* sync = wsb + (size_t)N * g.frame;
    const int R = rounds < 0 ? kJsDefaultRounds : rounds;
    const int stop = stages < 0 ? -stages : 0;               // for measurements: after the guess, the hand-over, the repair and scan
    if (g.mode == JD_MODE_420)
        rc = js_launch<JD_MODE_420>(in, in_stride, N, H, W, g, p.chunk, R, coef, coef_stride, status, sync, p.frame, p.nc_max, p.cpw, stats, stop, st);
    else if (g.mode == JD_MODE_444)
        rc = js_launch<JD_MODE_444>(in, in_stride, N, H, W, g, p.chunk, R, coef, coef_stride, status, sync, p.frame, p.nc_max, p.cpw, stats, stop, st);
    else
        rc = js_launch<JD_MODE_GREY>(in, in_stride, N, H, W, g, p.chunk, R, coef, coef_stride, status, sync, p.frame, p.nc_max, p.cpw, stats, stop, st);
    if (rc || stop) return rc;
    return mjpegd_launch_planes(g, H, W, in, in_stride, N, coef, coef_stride, wsb, out, row_stride, frame_stride, stages, stream);
}

/* See include/stabnet_hip.h: the same entropy launches, then the IDCT and the crop to the dense I420 frame. */
int stabnet_mjpeg_decode_sync_i420(const unsigned char* in, size_t in_stride, int N, int H, int W, int C, int subsampling, unsigned char* out,
                                   size_t frame_stride_bytes, int* status, void* workspace, size_t workspace_bytes, int chunk_bytes, int rounds,
                                   int* stats, void* stream, void* prof) {
    SN_REQUIRE(in && out && status && workspace, "mjpeg_decode_sync_i420: null pointer");
    JdGeom g;
    int rc = mjpegd_i420_geom("mjpeg_decode_sync_i420", N, H, W, C, subsampling, frame_stride_bytes, &g);
    if (rc) return rc;
    SN_REQUIRE(js_chunk(chunk_bytes), "mjpeg_decode_sync_i420: chunk_bytes %d is not 0 (default) or a multiple of 4 in 8..4096", chunk_bytes);
    SN_REQUIRE(rounds >= -1 && rounds <= 1024, "mjpeg_decode_sync_i420: rounds %d is not -1 (default) or 0..1024", rounds);
    SN_REQUIRE((in_stride & 15) == 0 && ((uintptr_t)in & 15) == 0, "mjpeg_decode_sync_i420: in and in_stride must be 16-byte aligned");
    JsPlan p;
    SN_REQUIRE(in_stride >= g.blob_max && js_plan(g, in_stride, chunk_bytes, &p), "mjpeg_decode_sync_i420: in_stride %zu < %zu (or 2^30 and above)",
               in_stride, g.blob_max);
    if (workspace_bytes < (size_t)N * (g.frame + p.frame)) {
        stabnet_set_error("mjpeg_decode_sync_i420: workspace %zu < %zu bytes", workspace_bytes, (size_t)N * (g.frame + p.frame));
        return STABNET_ERR_WORKSPACE;
    }
    SN_REQUIRE(((uintptr_t)workspace & 15) == 0, "mjpeg_decode_sync_i420: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    rc = sn_check_device(in, "mjpeg_decode_sync_i420: in", st);
    if (rc == 0) rc = sn_check_device(out, "mjpeg_decode_sync_i420: out", st);
    if (rc == 0) rc = sn_check_device(workspace, "mjpeg_decode_sync_i420: workspace", st);
    if (rc == 0) rc = sn_check_device(status, "mjpeg_decode_sync_i420: status", st);
    if (rc == 0 && stats) rc = sn_check_device(stats, "mjpeg_decode_sync_i420: stats", st);
    if (rc) return rc;
    unsigned char* wsb = static_cast<unsigned char*>(workspace);
    rc = mjpegd_clear_status(status, N, stream);
    if (rc) return rc;
    short* coef = reinterpret_cast<short*>(wsb + g.coef);
    const size_t coef_stride = g.frame / sizeof(short);
    unsigned char* sync = wsb + (size_t)N * g.frame;
    const int R = rounds < 0 ? kJsDefaultRounds : rounds;
    if (g.mode == JD_MODE_420)
        rc = js_launch<JD_MODE_420>(in, in_stride, N, H, W, g, p.chunk, R, coef, coef_stride, status, sync, p.frame, p.nc_max, p.cpw, stats, 0, st);
    else
        rc = js_launch<JD_MODE_GREY>(in, in_stride, N, H, W, g, p.chunk, R, coef, coef_stride, status, sync, p.frame, p.nc_max, p.cpw, stats, 0, st);
    if (rc) return rc;
    return mjpegd_launch_i420(g, H, W, in, in_stride, N, coef, coef_stride, wsb, out, frame_stride_bytes, stream, prof);
}

}  // extern "C"
