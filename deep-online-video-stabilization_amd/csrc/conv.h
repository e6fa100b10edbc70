// Internal launcher interface of the implicit-GEMM convolution kernels (conv.hip).
#pragma once
#include "common.h"

struct ConvArgs {
    // tensors
    const float* x;          // input  NHWC [N,H,W,Cin]
    const float* w;          // weights OHWI [Cout][KH][KW][Cin]   (row n = one output channel, K contiguous)
    float* y;                // output NHWC [N,Ho,Wo,Cout]
    const float* bias;       // [Cout] or null
    const float* in_scale;   // [Cin] or null: A-operand prologue  a = relu(a*scale + shift)  (folded BN + ReLU)
    const float* in_shift;   // [Cin]
    const float* residual;   // NHWC [N,res_H,res_W,Cout] or null; read at (oy*res_stride, ox*res_stride)
    const float* out_scale;  // [Cout] or null: epilogue  y = y*out_scale + out_shift  (folded BN of the CONSUMER, inference)
    const float* out_shift;
    const float* out_floor;  // [Cout] or null: with out_scale, y = max(y, out_floor[n]) instead of the relu_out flag (0 = ReLU,
                             // -inf = none): lets ONE launch produce channels with and without an activation
    float* partial;          // split-K workspace [splitk][M][Cout] (only when splitk > 1)
    // geometry
    int N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad;
    int up;                  // input dilation ("fractional stride") used by dgrad of strided convs; 1 otherwise
    int res_H, res_W, res_stride;
    int relu_out;
    int x_ld, res_ld;        // floats between consecutive pixels of x / of the residual (0 = Cin / Cout: dense tensors); the
                             // inference plan keeps two tensors side by side in one buffer (shortcut | conv1 of a projection unit)
    int M, K;                // M = N*Ho*Wo, K = KH*KW*Cin
    int splitk, steps_per_split;
    int cin_real;            // un-padded Cin (algorithmic flop accounting only); 0 = Cin
    unsigned div_hw_mul, div_hw_shift, div_w_mul, div_w_shift;   // exact m / (Ho*Wo) and r / Wo by multiply-high (conv_plan)
    int rowrun;              // 1: "row-run" A operand (ring kernel MODE 2, the 13-channel stem): for every filter row kh the KW*Cin
                             //    input floats of a tap row are contiguous; they are taken as ONE run, zero-padded to a multiple of 32,
                             //    so K = KH * roundup(KW*Cin, 32) and the weights are [Cout][KH][roundup(KW*Cin, 32)].  Cin is the
                             //    real (unpadded) pixel stride; no prologue.
    int in_scale_expected;   // plan-time hint: 1 if the launch will carry an input BN prologue (in_scale is bound later)
    int xcd_swizzle;         // 1: remap workgroup ids so each XCD (own 4 MiB L2) works on a contiguous run of M tiles
};

// Chooses tile shape / split-K and returns the workspace bytes the launch needs (0 if none).
size_t conv_plan(ConvArgs& a);
// Enqueues the convolution (and the split-K reduction when a.splitk > 1).
struct Prof;
// bf16_operands = 1: SECONDARY fast mode: A and B fragments are rounded to bf16 when they are read from
// LDS and multiplied by v_mfma_f32_32x32x16_bf16 (fp32 accumulate; tensors stay fp32 in memory).  Never the default: the
// reference is fp32 end to end.  (A launch argument, not a ConvArgs field: the fp32 kernels' argument block -- and with it their
// register allocation -- stays exactly what it was; an extra field cost the fp32 path 1 %.)
// bf16_operands = 2 / 3: split operands -- exact f32 products as six / nine bf16 MFMAs, both operands split when the fragments
// are read (conv_kernel.h, sn_split3).  bf16_operands = 4 with w_img: the weights come as a pre-split fragment-major image
// (conv_weight_image_floats / launch_weight_split_image), only the A fragments are split at run time; launches the packed ring
// kernel cannot take (register-staged path, in-workgroup split-K) run the exact f32 MFMA kernels on a.w as before.
// lowk_ring (with a weight image only): 1x1 launches over 64 input channels, which conv_route() otherwise keeps on the register-staged
// exact-f32 kernel (two K steps: more resident workgroups for the epilogues), take the packed split kernel as well.  The training
// step's dgrad asks for it, so that every stride-1 dgrad of a split-operand step runs one arithmetic; measured on the block-1 conv1
// dgrads of the 8 x 288 x 512 step (M = 147 456): 26.5 us packed against 27.8 us (64 channels out), 71 against 68 - 74 us (256 out).
int conv_launch(const ConvArgs& a, hipStream_t st, Prof* prof = nullptr, int bf16_operands = 0, const float* w_img = nullptr,
                bool lowk_ring = false);

// The range every conv launch is held to ("Conv extents"): the kernels reach their operands through 32-bit offsets from the
// operand's pointer -- BYTE offsets in the ring and back-to-back kernels (input, OHWI weights, the back-to-back residual), element
// offsets built from `int` products elsewhere -- so an operand's whole extent, ALL x_ld / res_ld columns of every pixel, stays below
// 2^30 floats.  One limit for every family: which kernel a launch runs depends on the operand mode and the fusions, its buffers do not.
constexpr long SN_CONV_EXTENT_LIMIT = 1L << 30;
// The first operand of the planned launch `a` (conv_plan() called, x_ld / res_ld final) that reaches the limit -- "input", "output",
// "residual" or "weights", null when all are inside; *floats = its extent.  in_floats: floats from a.x to the end of the buffer the
// input lives in (<= 0: the dense [N][H][W][x_ld] tensor; the plan passes its own, the row-run stem's bordered image too); has_residual: the
// launch reads one ([N][res_H][res_W][res_ld]).  Host only.
const char* conv_extent_over(const ConvArgs& a, long in_floats, bool has_residual, long* floats);

// Which kernel a convolution runs: decided ONCE, by conv_route(), for the launcher (conv_launch), for the plan's launch count and step
// info (net.hip) and for the Profiler's kernel name alike.
enum ConvFamily {
    CONV_IGEMM,        // register-staged conv_igemm_f32_kernel<tile, bk, ..., mode, nbuf, operand>
    CONV_RING,         // LDS-DMA ring, conv_ring_f32_kernel<mode, operand, 1, 0>
    CONV_RING_KG,      // ... K groups inside the workgroup: <mode, operand, 3, 0>, or <0, operand, 2, 1> with the fragment prologue
    CONV_RING_PRO,     // ... fragment prologue, <0, operand, 1, 1>
    CONV_PACKED,       // packed split kernel on the pre-split weight image, <mode, 4, 1, pro>
    CONV_PACKED_KG2,   // ... two K groups inside the workgroup, <mode, 4, 2, pro>
    CONV_ASTAT,        // A-stationary packed kernel (conv_astat_kernel.h), conv_astat_f32_kernel<astat_bm>: the wide 1x1 launches over
                       // K <= 256 that CONV_PACKED would take without a K split -- the same arithmetic, bit for bit
    CONV_PATCH         // patch-stationary packed kernel (conv_patch_kernel.h), conv_patch_f32_kernel<8, 8, WR, 3>: the 3x3 / pad 1 / stride 1
                       // launches over large maps that CONV_PACKED would take without a K split -- the same arithmetic, bit for bit
};
struct ConvRoute {
    int family;        // ConvFamily
    int tile, bk, nbuf;   // CONV_IGEMM: TileId (conv.hip), K-step, LDS stages
    int mode;          // the kernels' MODE argument: 0 unpadded, 1 zero padding, 2 row-run (ring) / dilated input (register-staged)
    int operand;       // the kernels' BF16 argument actually run (operand mode 4 runs 0 wherever the packed kernel does not take the launch)
    int kg, pro;       // ring kernels: K groups inside the workgroup, fragment prologue
    int reduce;        // 1: a split-K reduce launch follows
    int prof_kind;     // PK_KERNEL_CONV_* (prof.h)
    int astat_bm;      // CONV_ASTAT: rows of M per workgroup (the kernel's BM: 32 is the one instantiation built)
    int patch_cfg;     // CONV_PATCH: the kernel's form, 1 = <8, 8, 1, 3> (8 x 8 pixels, a wave per 32 x 32 tile), 2 = <8, 8, 2, 3> (a wave
                       // multiplies both 32-row blocks of the patch with one B fragment)
};
// operand_mode: conv_launch's bf16_operands; has_image: the launch comes with a pre-split weight image (mode 4 without one is mode 0).
// The pointers of `a` are the launch's: a prologue is a.in_scale != null, and out_scale, out_floor and partial are looked at (never
// through).  Host code that asks before memory exists binds placeholders (sn_placeholder_base).  Reads nothing but its arguments, the
// once-per-process STABNET_CONV_* switches and the tuning hooks (stabnet_conv_tuning_*).
ConvRoute conv_route(const ConvArgs& a, int operand_mode, bool has_image, bool lowk_ring = false /* see conv_launch() */);
// Base pointers for host code that wants the launcher's view of a launch whose memory does not exist yet: base k = k << 40, far enough
// apart that no two pointers bound to different bases meet; never dereferenced.
static inline float* sn_placeholder_base(int k) { return reinterpret_cast<float*>((size_t)k << 40); }
// The grid of the conv launch of route `r` on a chip of `cus` CUs (less the reserved ones, stabnet_conv_reserve_cus): the ONE rule the
// launchers size their grids by.  tiles = units of work the workgroups walk: (M tile, N tile, K slice) of the 64 x 64 kernels (K
// groups inside the workgroup are no tiles), (M tile | patch, pass over the column blocks its waves take side by side) of the
// A-stationary and patch kernels; wgs = gx * gy * gz workgroups.  Host only: reads no device.
struct ConvGrid { long tiles, wgs; int gx, gy, gz; };
ConvGrid conv_grid(const ConvRoute& r, const ConvArgs& a, int cus);
// LDS the A-stationary kernel's planes / the patch kernel's launch take for `a`, and the limits the launchers hold them to
size_t conv_astat_plane_bytes(const ConvRoute& r, const ConvArgs& a);
size_t conv_astat_plane_limit();
size_t conv_patch_lds_bytes(const ConvRoute& r, const ConvArgs& a);
size_t conv_patch_lds_limit();
int conv_plan_total_steps(const ConvArgs& a);   // K-steps of the whole reduction (all slices)
// Kernel name of a PK_KERNEL_CONV_* Profiler kind as rocprofv3 prints the instantiation; null for any other kind.
const char* conv_prof_kind_name(int kind);
// Pre-split weight image of a convolution whose weights are [Cout][K] rows (K % 32 == 0): per (64-channel N tile, 32-deep K step)
// 3072 floats = [wave column 2][plane h, m, l][k group 2][lane 64][8 bf16]; lane (n = lane & 31, g = lane >> 5), element e holds
// k = 32 step + 16 group + 8 (e >> 2) + 4 g + (e & 3) -- the k order of the ring kernel's A fragments.
size_t conv_weight_image_floats(int Cout, int K);
int launch_weight_split_image(const float* w, int Cout, int K, float* img, hipStream_t st);
// The images of several weight matrices by ONE launch (the training step re-splits its dgrad weights once per step): matrix i is
// w_base[w_off[i] ...] as [Cout[i]][K[i]], its image goes to img_base[img_off[i] ...]; tprefix = running thread counts.
struct WeightImageTable { long w_off[64], img_off[64], tprefix[65]; int Cout[64], K[64]; int n; };
void weight_image_table_add(WeightImageTable& t, long w_off, long img_off, int Cout, int K);
int launch_weight_split_images(const float* w_base, float* img_base, const WeightImageTable& t, hipStream_t st);

// The two siamese towers of a training step as ONE launch (forward convolutions, conv_kernel.h).  `a` describes the pair as one
// batch of 2N samples whose first N live where a.x / a.y / a.residual / a.in_scale / a.in_shift point; tiles of rows >= m_tower
// (the second tower: its tensors sit in another workspace, and its batch statistics differ) get these ELEMENT offsets added to
// the five pointers.  m_tower must be a multiple of the tile height (64).  conv_pair_supported(): the plan of `a` is a 64x64
// register-staged launch (anything else: launch the towers one after the other).
struct ConvPair { int m_tower, x_tower_floats /* N*H*W*Cin of one tower's input */; long dx, dy, dres, dscale; };
bool conv_pair_supported(const ConvArgs& a);
int conv_launch_pair(const ConvArgs& a, const ConvPair& pr, hipStream_t st, Prof* prof = nullptr,
                     const float* w_img = nullptr /* pre-split image of a.w: the prologue-carrying 1x1 pairs run the packed split kernel */);

// A bottleneck unit's 3x3 `conv2` and 1x1 `conv3` as ONE launch (conv_b2b_kernel.h): c2 / c3 are the two planned convolutions as
// conv_launch() would take them (c2.out_scale / out_shift = the folded BN between them, ReLU implied; c2.y is not written).
// conv_b2b_supported(): the geometry the kernel takes (3x3 / pad 1 over Cin == Cout == 64 or 128, no bias / residual / prologue;
// 1x1 stride-1 c3 over the same pixels with Cout a multiple of c2.Cout, no prologue) -- pointers are not looked at.
bool conv_b2b_supported(const ConvArgs& c2, const ConvArgs& c3);
int conv_b2b_launch(const ConvArgs& c2, const ConvArgs& c3, hipStream_t st, Prof* prof = nullptr);

// A unit's 1x1 `conv3` (+ bias + residual) and the next identity unit's 1x1 `conv1` as ONE launch (conv_pair_kernel.h): c3 / c1 are the
// two planned convolutions as conv_launch() would take them in operand mode 4 (c1.in_scale / in_shift = the pre-activation between them,
// c1.x is not read: it is c3.y).  conv_unit_pair_form(): the kernel's form for the pair, false if it does not take it -- both 1x1 / stride 1
// / pad 0 over the same pixels without a K split, c1.Cin == c3.Cout a multiple of 128, a plain residual (stride 1, same map), c1.Cout 64
// (BM = 64) or 128 (BM = 32), c3.K a multiple of 64 up to 256 with A tile + chunk within conv_unit_pair_lds_limit(), AND conv_route() sending the two launches to the kernels whose
// arithmetic the fused kernel repeats: c3 to the exact-f32 register-staged kernel over 64 channels (f32 form, no image needed) or to a
// packed kernel without prologue / K groups (packed form), c1 to the packed prologue kernel.  Pointers as in conv_route().
struct ConvUnitPairForm { int f32a, bm; int prof_kind; size_t lds_bytes; };
bool conv_unit_pair_form(const ConvArgs& c3, const ConvArgs& c1, bool img3, bool img1, ConvUnitPairForm& f);
size_t conv_unit_pair_lds_limit();
ConvGrid conv_unit_pair_grid(const ConvUnitPairForm& f, const ConvArgs& c3);
int conv_unit_pair_launch(const ConvArgs& c3, const ConvArgs& c1, const float* w3_img, const float* w1_img, hipStream_t st, Prof* prof = nullptr);

// Exact unsigned division by an invariant divisor d >= 1 for numerators n < 2^31 (Granlund-Montgomery round-up form):
//   l = ceil(log2 d), mul = floor(2^32 (2^l - d) / d) + 1, n / d = (mulhi(mul, n) + n) >> l.
// Three instructions instead of the ~40 of a software 32-bit division; the kernels' per-tile index setup is VALU work
// that competes with the MFMAs for issue slots.
static inline void sn_fastdiv_make(unsigned d, unsigned& mul, unsigned& shift) {
    unsigned l = 0;
    while ((1ull << l) < d) ++l;
    mul = (unsigned)((((1ull << l) - d) << 32) / d + 1);
    shift = l;
}
#ifdef __HIPCC__
__device__ __forceinline__ int sn_fastdiv(int n, unsigned mul, unsigned shift) {
    return (int)((__umulhi(mul, (unsigned)n) + (unsigned)n) >> shift);
}
#endif
