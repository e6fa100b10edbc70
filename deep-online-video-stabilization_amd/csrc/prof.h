// Optional per-launch HIP-event instrumentation used by bench.py's roofline leg (never on by default).
#pragma once
#include <vector>
#include "common.h"

enum {
    PK_KERNEL_PAD = 1, PK_KERNEL_POOL = 2, PK_KERNEL_GAP = 3, PK_KERNEL_FC = 4, PK_KERNEL_MESH = 5,
    PK_KERNEL_WARP = 6, PK_KERNEL_ASSEMBLE = 7, PK_KERNEL_PUSH = 8, PK_KERNEL_SPLITK_REDUCE = 9, PK_KERNEL_WGRAD = 10, PK_KERNEL_HEAD = 20,
    PK_KERNEL_MJPEG_TRANSFORM = 30, PK_KERNEL_MJPEG_ENTROPY = 31, PK_KERNEL_MJPEG_LAYOUT = 32, PK_KERNEL_MJPEG_GATHER = 33 /* mjpeg.hip; bytes = what the shapes fix, the compressed bytes come on top */,
    PK_KERNEL_INGEST_GREY_ROWS = 34, PK_KERNEL_INGEST_GREY_COLS = 35, PK_KERNEL_INGEST_COLOUR = 36 /* ingest.hip; bytes = source rows read + intermediate + output */,
    PK_KERNEL_MAP_SHRINK = 37, PK_KERNEL_REMAP_SRC = 38, PK_KERNEL_REMAP_SRC4 = 39 /* remap.hip, stabnet_warp_rev_bundle2_src; bytes = frame gathered + frame written + small maps */,
    PK_KERNEL_REMAP_WIN = 60, PK_KERNEL_REMAP_WIN4 = 61 /* remap.hip, stabnet_warp_rev_bundle2_win; bytes = window gathered + output written + small maps */,
    PK_KERNEL_REMAP_WIN_DEV = 62, PK_KERNEL_REMAP_WIN4_DEV = 63 /* remap.hip, stabnet_warp_rev_bundle2_win_dev; bytes = whole frame (the window is on the device) + output written + small maps */,
    PK_KERNEL_REMAP_I420 = 59 /* remap.hip, stabnet_warp_rev_bundle2_i420; bytes = the window of every plane gathered + the planes written + small maps */,
    PK_KERNEL_REMAP_CUBIC = 250 /* + 2 * window_kind + (four-pixel path): remap_cubic_kernel<PX, KIND>, stabnet_warp_rev_bundle2_cubic; bytes as the bilinear kind's */,
    PK_KERNEL_REMAP_I420_CUBIC = 256 /* remap_i420_kernel<true>; bytes as PK_KERNEL_REMAP_I420 */,
    PK_KERNEL_MJPEGD_PLANES = 257 /* mjpeg_decode.hip, stabnet_mjpeg_decode_i420 / _sync_i420; bytes = the planes read + the I420 frame written */,
    PK_KERNEL_MJPEG_TRANSFORM_PLANAR = 258 /* mjpeg.hip, stabnet_mjpeg_encode_i420; bytes = the I420 frame read + the coefficients written */,
    PK_KERNEL_TF_GET_IMG = 64/* tf_image.hip; bytes = 12 tap bytes read + 4 written per destination value, every channel named */,
    PK_KERNEL_TVL1_STEP = 57, PK_KERNEL_TVL1_FUSED = 58 /* tvl1.hip, one record per launch; bytes = ten planes read + six written once, shape[0] = sweeps of the launch */,
    PK_KERNEL_TVL1_DOWN = 65, PK_KERNEL_TVL1_GRAD = 66, PK_KERNEL_TVL1_WARP = 67, PK_KERNEL_TVL1_UP = 68, PK_KERNEL_TVL1_MAP = 69 /* tvl1.hip stages; bytes = every plane read or written, once */,
    PK_KERNEL_KLT_DETECT = 26, PK_KERNEL_KLT_TRACK = 27, PK_KERNEL_KLT_FINISH = 28 /* klt.hip; bytes = detect: the image once; track: 16 per bilinear sample (gathers, mostly from L2), shape[0] = iterations; finish: the cell and row records */,
    PK_KERNEL_HOMFIT = 29 /* homfit.hip; bytes = the rows once + the mask + the small outputs, shape[0] = hypotheses */,
    PK_KERNEL_WGRAD_SAME = 11 /* + 2*K3 + PRO, + 4 with the bias sums (K3 = 0): conv_wgrad_same_f32_kernel<K3, PRO, BIAS> */,
    PK_KERNEL_CONV_PAIR = 80 /* + 2*MODE + (BK==32): conv_igemm_f32_pair_kernel<64, 64, BK, 32, 32, MODE> */, PK_KERNEL_CONV_KG = 84 /* + mode: conv_ring_f32_kernel<MODE, 0, 3, 0>; + 2: conv_ring_f32_kernel<0, 0, 1, 1> (fragment prologue); + 3: <0, 0, 2, 1> */, PK_KERNEL_CONV_RING = 90 /* + mode; + 3 for the bf16-operand variants */,
    PK_KERNEL_CONV_PACKED = 70 /* + mode: conv_ring_f32_kernel<MODE, 4, 1, 0> (pre-split weight image); + 3: <0, 4, 1, 1>; + 4 + mode: <MODE, 4, 2, 0>; + 6: <0, 4, 2, 1> */,
    PK_KERNEL_CONV_ASTAT = 77 /* conv_astat_f32_kernel<32> */,
    PK_KERNEL_CONV_PATCH = 24 /* + 0: conv_patch_f32_kernel<8, 8, 1, 3>; + 1: <8, 8, 2, 3> (ConvRoute::patch_cfg - 1) */,
    PK_KERNEL_CONV_B2B = 96 /* conv_b2b_f32_kernel<2>; + 1: <4> */,
    PK_KERNEL_CONV_UNIT_PAIR = 244 /* + 2 * F32A + (BM == 64): conv_unit_pair_f32_kernel<F32A, BM> (conv_pair_kernel.h) */,
    PK_KERNEL_CONV_SPLIT = 40 /* + 8 * (BF16 - 2) + slot, the read-time split modes 2 / 3: conv_ring_f32_kernel<MODE, BF16, KG, PRO>, slot 0..2 = <MODE, B, 1, 0>,
                                 3 / 4 = <0 / 1, B, 3, 0>, 5 = <0, B, 1, 1>, 6 = <0, B, 2, 1> */,
    PK_KERNEL_CONV_BASE = 100   // + MODE*6 + tile*2 + (BK==32) + 18 if NBUF == 1 + 36 * BF16 (conv_igemm_f32_kernel<..., NBUF, BF16>, BF16 0..3)
};

struct Prof {
    std::vector<hipEvent_t> ev;     // 2 per record
    std::vector<int> kind;
    std::vector<double> flops, bytes;
    std::vector<int> shape;         // 4 ints per record: M, N, K, split-K (0 when not a GEMM)
    int cap = 0, n = 0;
    bool begin(hipStream_t st) {
        if (n >= cap) return false;
        (void)hipEventRecord(ev[2 * n], st);
        return true;
    }
    void end(hipStream_t st, int k, double f, double b, int sm = 0, int sn = 0, int sk = 0, int ss = 0) {
        (void)hipEventRecord(ev[2 * n + 1], st);
        kind[n] = k; flops[n] = f; bytes[n] = b;
        shape[4 * n] = sm; shape[4 * n + 1] = sn; shape[4 * n + 2] = sk; shape[4 * n + 3] = ss;
        ++n;
    }
};
