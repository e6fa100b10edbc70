// The reference's get_img (get_data_mini_after.py:149-156) behind the JPEG decoder: decoded uint8 BGR frames of any size to the
// channels of the training tensors stable [N,H,W,14] / unstable [N,H,W,2], in ONE launch per destination tensor.
//   tf.image.rgb_to_grayscale -> convert_image_dtype(float32) -> resize_images(method=0) -> - 0.5
// [external] TensorFlow 1.3's arithmetic, restated (TensorFlow is not a dependency; tests/tf_image_model.py is the same restatement
// in NumPy and the yardstick):
//   c   = float(u8) * float(1/255)                       per colour, convert_image_dtype uint8 -> float32
//   s   = (r*0.2989f + g*0.5870f) + b*0.1140f            rgb_to_grayscale: summed left to right, every product and sum rounded
//   u   = uint8(trunc(s * 255.5f))                       convert_image_dtype float32 -> uint8 (rgb_to_grayscale returns its input's type)
//   f   = float(u) * float(1/255)                        get_img's own convert_image_dtype
//   legacy bilinear resize (align_corners = False, no half-pixel centres): scale = float(in) / float(out), in_y = float(y) * scale,
//   top = floor(in_y), bottom = in_y < in - 1 ? ceil(in_y) : in - 1, lerp = in_y - floor(in_y); rows first:
//   t = tl + (tr - tl) * xl, b = bl + (br - bl) * xl, out = t + (b - t) * yl; then - 0.5f.
// The grey sum is order-sensitive (47 of the 2^24 triples change their byte when summed right to left), so every operation is an
// explicitly rounded __fmul_rn / __fadd_rn / __fsub_rn: nothing here may be contracted into an fma or reassociated.
// The launch is organised by DESTINATION: a workgroup owns kThreads consecutive pixels of one pair n -- in NHWC those are
// kThreads * C consecutive floats --, walks the pair's C channels (each names its own source frame), gathers 4 taps x 3 bytes per
// value, collects the values in LDS as [pixel][channel] and stores the tile as dense rows of dwords.  A channel no entry names is
// skipped by the store, so it keeps what it held.  No atomics, no workspace, no host copy: the launch can sit in a captured graph.
#include "common.h"
#include "prof.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxC = 32;                // channels of the destination: kThreads * kMaxC floats = 32 KB of LDS
constexpr int kFields = 6;               // int64 per table entry: byte offset, sh, sw, row stride in bytes, n, c
constexpr long long kMaxSide = 65536;    // of a source frame and of the destination: keeps every product below 2^63 and float(y) exact

__device__ __forceinline__ float tf_grey(const unsigned char* __restrict__ px) {          // px: B, G, R as the decoder writes them
    const float k = 1.0f / 255.0f;
    const float b = __fmul_rn((float)px[0], k), g = __fmul_rn((float)px[1], k), r = __fmul_rn((float)px[2], k);
    const float s = __fadd_rn(__fadd_rn(__fmul_rn(r, 0.2989f), __fmul_rn(g, 0.5870f)), __fmul_rn(b, 0.1140f));
    int u = (int)__fmul_rn(s, 255.5f);                                                     // s >= 0: the cast truncates
    u = u > 255 ? 255 : u;                                                                 // saturate_cast (never reached: s < 1)
    return __fmul_rn((float)u, k);
}

// One axis of the legacy resize for output index o.
__device__ __forceinline__ void tf_axis(int o, int in, float scale, int* lo, int* hi, float* lerp) {
    const float f = __fmul_rn((float)o, scale), fl = floorf(f);
    int a = (int)fl, b = f < (float)(in - 1) ? (int)ceilf(f) : in - 1;
    *lerp = __fsub_rn(f, fl);
    *lo = a < in - 1 ? a : in - 1;                                                         // (a <= in - 1 already: the clamps only bound the reads)
    *hi = b < in - 1 ? b : in - 1;
}

// grid (cdiv(H * W, kThreads), N)
__global__ __launch_bounds__(kThreads) void tf_get_img_kernel(const unsigned char* __restrict__ frames, long long frames_bytes,
                                                               const long long* __restrict__ table, int n_entries,
                                                               float* __restrict__ dst, int H, int W, int C) {
    extern __shared__ float vals[];                                                        // [kThreads][C]
    __shared__ int ent[kMaxC];                                                             // the entry of channel c of this pair, -1: none
    const int n = blockIdx.y;
    if ((int)threadIdx.x < C) {
        int found = -1;
        for (int e = 0; e < n_entries; ++e) {                                              // the last entry that names (n, c) wins
            const long long* t = table + (size_t)e * kFields;
            if (t[4] != n || t[5] != (long long)threadIdx.x) continue;
            const long long off = t[0], sh = t[1], sw = t[2], rs = t[3];
            // an entry whose frame does not lie inside `frames` is not followed: nothing is read out of bounds
            const bool ok = off >= 0 && sh >= 1 && sw >= 1 && sh <= kMaxSide && sw <= kMaxSide && rs >= 3 * sw && rs <= (1LL << 31) &&
                            off <= frames_bytes && (sh - 1) * rs + 3 * sw <= frames_bytes - off;
            found = ok ? e : -1;
        }
        ent[threadIdx.x] = found;
    }
    __syncthreads();
    const long long HW = (long long)H * W, p0 = (long long)blockIdx.x * kThreads, p = p0 + threadIdx.x;
    if (p < HW) {
        const int y = (int)(p / W), x = (int)(p % W);
        for (int c = 0; c < C; ++c) {
            const int e = ent[c];                                                          // uniform over the workgroup
            if (e < 0) continue;
            const long long* t = table + (size_t)e * kFields;
            const int sh = (int)t[1], sw = (int)t[2];
            const long long rs = t[3];
            const unsigned char* f = frames + t[0];
            int y0, y1, x0, x1;
            float yl, xl;
            tf_axis(y, sh, __fdiv_rn((float)sh, (float)H), &y0, &y1, &yl);
            tf_axis(x, sw, __fdiv_rn((float)sw, (float)W), &x0, &x1, &xl);
            const unsigned char* r0 = f + (size_t)y0 * rs;
            const unsigned char* r1 = f + (size_t)y1 * rs;
            const float tl = tf_grey(r0 + 3 * x0), tr = tf_grey(r0 + 3 * x1), bl = tf_grey(r1 + 3 * x0), br = tf_grey(r1 + 3 * x1);
            const float top = __fadd_rn(tl, __fmul_rn(__fsub_rn(tr, tl), xl));
            const float bot = __fadd_rn(bl, __fmul_rn(__fsub_rn(br, bl), xl));
            vals[threadIdx.x * C + c] = __fsub_rn(__fadd_rn(top, __fmul_rn(__fsub_rn(bot, top), yl)), 0.5f);
        }
    }
    __syncthreads();
    const long long left = HW - p0;
    const int count = (int)(left < kThreads ? left : kThreads) * C;                        // floats of this tile: consecutive in dst
    float* o = dst + ((size_t)n * HW + p0) * C;
    for (int j = threadIdx.x; j < count; j += kThreads)
        if (ent[j % C] >= 0) o[j] = vals[j];
}

}  // namespace

extern "C" {

int stabnet_tf_get_img(const unsigned char* frames_u8, size_t frames_bytes, const int64_t* table_dev, int n_entries, float* dst, int N,
                       int H, int W, int C, void* stream, void* profp) {
    SN_REQUIRE(frames_u8 && table_dev && dst, "tf_get_img: null pointer");
    SN_REQUIRE(frames_bytes >= 3 && frames_bytes <= (size_t)1 << 62, "tf_get_img: frames_bytes %zu holds no pixel", frames_bytes);
    SN_REQUIRE(n_entries >= 1 && n_entries <= 1 << 20, "tf_get_img: n_entries must be 1..2^20, got %d", n_entries);
    SN_REQUIRE(N >= 1 && N <= 65535, "tf_get_img: N must be 1..65535, got %d", N);
    SN_REQUIRE(H >= 1 && W >= 1 && H <= kMaxSide && W <= kMaxSide, "tf_get_img: H and W must be 1..65536, got %d x %d", H, W);
    SN_REQUIRE(C >= 1 && C <= kMaxC, "tf_get_img: C must be 1..%d, got %d", kMaxC, C);
    hipStream_t st = (hipStream_t)stream;
    int rc = sn_check_device(frames_u8, "tf_get_img: frames_u8", st);
    if (rc == 0) rc = sn_check_device(table_dev, "tf_get_img: table_dev", st);
    if (rc == 0) rc = sn_check_device(dst, "tf_get_img: dst", st);
    if (rc) return rc;
    Prof* prof = static_cast<Prof*>(profp);
    const bool rec = prof && prof->begin(st);
    tf_get_img_kernel<<<dim3(cdiv((long)H * W, kThreads), N), kThreads, (size_t)kThreads * C * sizeof(float), st>>>(
        frames_u8, (long long)frames_bytes, reinterpret_cast<const long long*>(table_dev), n_entries, dst, H, W, C);
    // the table lives on the device: the bytes are those of a launch that names every channel, 12 tap bytes + 4 written per value
    if (rec) prof->end(st, PK_KERNEL_TF_GET_IMG, 0.0, (double)N * H * W * C * 16.0);
    SN_LAUNCH_CHECK("tf_get_img_kernel");
    return STABNET_OK;
}

}  // extern "C"
