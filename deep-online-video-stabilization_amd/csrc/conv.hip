// Implicit-GEMM convolution on the gfx950 matrix cores, exact float32 (v_mfma_f32_32x32x2_f32).
//
//   y[m][n] = sum_k A(m,k) * Wt[n][k]      m = (img, oy, ox)   k = (kh, kw, c)   n = output channel
//   A(m,k)  = act( x[img, oy*stride-pad+kh, ox*stride-pad+kw, c] )   act = optional folded BN + ReLU (prologue)
//
// Replaces the slim conv2d / conv2d_same (+ batch_norm + relu) clusters of resnet_v2_50 called at
// s_net_bundle_nobm.py:252-253 (SURVEY.md section 2.1 rows K1,K3,K4,K5).
//
// Tiling: 256 threads = 4 waves (64 lanes).  Block tile BM x BN, K-step BK; both operands are staged in LDS with
// the reduction index contiguous ([row][BK+4] floats, rows 16-B aligned, pitch 36/20 dwords = conflict-free
// ds_read_b128 for the 16-lane service groups).  Lane (i = lane&31, h = lane>>5) of a wave reads FOUR consecutive
// k (one ds_read_b128) of row i at k-offset 8*kk + 4*h and feeds them to four successive MFMAs: the MFMA's two
// k-slots are thus k = 8kk+e and 8kk+4+e for A and B alike -- a permutation of the reduction order only.
// Global->LDS staging goes through registers (the BN+ReLU prologue and the im2col zero padding need the VALU),
// issued one K-step ahead of the MFMAs (double-buffered LDS, one barrier per K-step).
#include "conv.h"
#include "prof.h"
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <string>
#include <vector>

#include "conv_kernel.h"
#include "conv_ring_kernel.h"
#include "conv_astat_kernel.h"
#include "conv_patch_kernel.h"
#include "conv_b2b_kernel.h"
#include "conv_pair_kernel.h"

// Sums the split-K partial slabs in a fixed order and applies the epilogue.  One thread per 4 channels.
template <int PAIR>
__device__ __forceinline__ void conv_splitk_reduce_body(const ConvArgs& p, const ConvPair& pr) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int c4n = p.Cout / 4;
    if (q >= (size_t)p.M * c4n) return;
    const int m = (int)(q / c4n);
    const int n = (int)(q - (size_t)m * c4n) * 4;
    const bool t1 = PAIR && m >= pr.m_tower;              // row of the second tower: its y / residual live at an offset
    const size_t slab = (size_t)p.M * p.Cout;
    const float* src = p.partial + (size_t)m * p.Cout + n;
    float4 s = *reinterpret_cast<const float4*>(src);
    for (int z = 1; z < p.splitk; ++z) {
        const float4 t = *reinterpret_cast<const float4*>(src + z * slab);
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    if (p.bias != nullptr) {
        const float4 b = *reinterpret_cast<const float4*>(p.bias + n);
        s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
    }
    if (p.residual != nullptr) {
        size_t ri;
        if (p.res_stride == 1 && p.res_H == p.Ho && p.res_W == p.Wo) {
            ri = (size_t)m * p.res_ld + n;
        } else {
            const int img = sn_fastdiv(m, p.div_hw_mul, p.div_hw_shift);
            const int rr = m - img * (p.Ho * p.Wo);
            const int oy = sn_fastdiv(rr, p.div_w_mul, p.div_w_shift), ox = rr - oy * p.Wo;
            ri = (((size_t)img * p.res_H + oy * p.res_stride) * p.res_W + ox * p.res_stride) * p.res_ld + n;
        }
        const float4 t = *reinterpret_cast<const float4*>(p.residual + (t1 ? pr.dres : 0) + ri);
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    if (p.out_scale != nullptr) {
        const float4 a = *reinterpret_cast<const float4*>(p.out_scale + n), b = *reinterpret_cast<const float4*>(p.out_shift + n);
        s.x = __builtin_fmaf(s.x, a.x, b.x); s.y = __builtin_fmaf(s.y, a.y, b.y);
        s.z = __builtin_fmaf(s.z, a.z, b.z); s.w = __builtin_fmaf(s.w, a.w, b.w);
    }
    if (p.out_scale != nullptr && p.out_floor != nullptr) {
        const float4 f = *reinterpret_cast<const float4*>(p.out_floor + n);
        s.x = fmaxf(s.x, f.x); s.y = fmaxf(s.y, f.y); s.z = fmaxf(s.z, f.z); s.w = fmaxf(s.w, f.w);
    } else if (p.relu_out) {
        s.x = fmaxf(s.x, 0.f); s.y = fmaxf(s.y, 0.f); s.z = fmaxf(s.z, 0.f); s.w = fmaxf(s.w, 0.f);
    }
    *reinterpret_cast<float4*>(p.y + (t1 ? pr.dy : 0) + (size_t)m * p.Cout + n) = s;
}
__global__ __launch_bounds__(256) void conv_splitk_reduce_kernel(const ConvArgs p) {
    conv_splitk_reduce_body<0>(p, ConvPair{});
}
__global__ __launch_bounds__(256) void conv_splitk_reduce_pair_kernel(const ConvArgs p, const ConvPair pr) {
    conv_splitk_reduce_body<1>(p, pr);
}

// ---------------------------------------------------------------------------------------------------------
enum TileId { T128x128 = 0, T128x64 = 1, T64x64 = 2 };

static void tile_dims(int t, int& bm, int& bn) {
    bm = (t == T64x64) ? 64 : 128;
    bn = (t == T128x128) ? 128 : 64;
}

static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

// Every environment switch of this file, read once per process (on first use).
struct ConvSwitches {
    int tile = env_int("STABNET_CONV_TILE", -1), splitk = env_int("STABNET_CONV_SPLITK", -1);   // forced tile / split-K (< 0: the built-in choice)
    int bk16 = env_int("STABNET_CONV_BK16", 0);
    int nbuf = env_int("STABNET_CONV_NBUF", 0);                      // register-staged kernel's LDS stages: 0 the rule, 1 / 2 forced
    int tuning_table = env_int("STABNET_CONV_TUNING_TABLE", 1);
    int split_below = env_int("STABNET_CONV_SPLIT_BELOW", 400), split_target = env_int("STABNET_CONV_SPLIT_TARGET", 448);
    int xcd = env_int("STABNET_CONV_XCD", 1);                        // halves the memory-side traffic at ~0.5 % of the frame rate
    int ring = env_int("STABNET_CONV_RING", 1), ring_wgs_per_cu = env_int("STABNET_CONV_RING_WGS_PER_CU", 3);   // 48 KiB of LDS each
    int lowk_igemm = env_int("STABNET_CONV_LOWK_IGEMM", 1);
    int ring_pro = env_int("STABNET_CONV_RING_PRO", 1);
    int kgroups = env_int("STABNET_CONV_KGROUPS", 1), kgroups_pro = env_int("STABNET_CONV_KGROUPS_PRO", 1);
    int packed_kg2 = env_int("STABNET_CONV_PACKED_KG2", 1), packed_kg3 = env_int("STABNET_CONV_PACKED_KG3", 1);
    int packed_pro = env_int("STABNET_CONV_PACKED_PRO", 1);
    int packed_wgs_per_cu = env_int("STABNET_CONV_PACKED_WGS_PER_CU", 2);                        // 60 KiB of LDS each
    // A-stationary packed kernel: on / off; the smallest M it takes (0: the rule in conv_route(), never below 2048) and the smallest
    // Cout (tests lower both to reach the kernel with small shapes)
    int astat = env_int("STABNET_CONV_ASTAT", 1), astat_min_m = env_int("STABNET_CONV_ASTAT_MIN_M", 0);
    int astat_min_cout = env_int("STABNET_CONV_ASTAT_MIN_COUT", 256);
    // patch-stationary packed kernel (3x3 / pad 1 / stride 1): on / off; the smallest M it takes (0: the rule in conv_route(), tests
    // lower it to reach the kernel with small shapes); its form (0: the rule in patch_cfg(), 1 / 2: ConvRoute::patch_cfg where it fits)
    int patch = env_int("STABNET_CONV_PATCH", 1), patch_min_m = env_int("STABNET_CONV_PATCH_MIN_M", 0);
    int patch_cfg = env_int("STABNET_CONV_PATCH_CFG", 0);
    int b2b = env_int("STABNET_CONV_B2B", 1), b2b_wgs_per_cu = env_int("STABNET_CONV_B2B_WGS_PER_CU", 2);   // 80 KB of LDS each
    int unit_pair = env_int("STABNET_CONV_PAIR", 1);               // 0: no pair of launches is fused (conv_unit_pair_form() refuses)
};
static const ConvSwitches& sw() {
    static const ConvSwitches s;
    return s;
}

// tuning hook (stabnet_conv_tuning_override, tools/autotune.py); tile -2: never called, the environment's choice holds
static int g_force_tile = -2, g_force_split = -1;
static int force_tile() { return g_force_tile == -2 ? sw().tile : g_force_tile; }
static int force_split() { return g_force_tile == -2 ? sw().splitk : g_force_split; }

static int conv_bk(const ConvArgs& a) { return (a.rowrun || (a.Cin % 32 == 0 && !sw().bk16)) ? 32 : 16; }
static int conv_total_steps(const ConvArgs& a) {
    if (a.rowrun) return a.KH * cdiv(a.KW * a.Cin, 32);
    return a.KH * a.KW * (a.Cin / conv_bk(a));
}

// ---- measured split-K table ------------------------------------------------------------------------------------
struct TuneEntry { int M, Cout, K, KH, ring, splitk; };
#include "conv_tuning_table.h"          // static const TuneEntry g_tuning_builtin[]; generated by tools/tune_splitk.py
#include "conv_tuning_table_packed.h"   // static const TuneEntry g_tuning_packed[]: the same measurement with the packed split kernels (operand mode 4)
static int g_tuning_profile = 0;        // 1: plans are made for the packed split kernels (stabnet_conv_tuning_profile)
static std::vector<TuneEntry> g_tuning_runtime;      // set through stabnet_conv_tuning_table_set (the tuner itself)

static int tuning_lookup(int M, int Cout, int K, int KH, int ring) {
    for (const TuneEntry& e : g_tuning_runtime)
        if (e.M == M && e.Cout == Cout && e.K == K && e.KH == KH && e.ring == ring) return e.splitk;
    if (sw().tuning_table && g_tuning_profile == 1)
        for (const TuneEntry& e : g_tuning_packed)
            if (e.M == M && e.Cout == Cout && e.K == K && e.KH == KH && e.ring == ring) return e.splitk;
    if (sw().tuning_table)
        for (const TuneEntry& e : g_tuning_builtin)
            if (e.M == M && e.Cout == Cout && e.K == K && e.KH == KH && e.ring == ring) return e.splitk;
    return 0;
}

static int pick_tile(const ConvArgs& a, int& splitk) {
    if (force_tile() >= 0) {
        const int steps0 = conv_total_steps(a);
        splitk = force_split() > 0 ? std::min(force_split(), steps0) : 1;
        return force_tile();
    }
    // Tile: at every shape of the regressor -- batch-1 720p, batch-8 288x512 forward and dgrad -- the 64x64 tile is the
    // fastest (tools/autotune.py, profiles/r01_autotune_*.txt).  Split-K: (1) the measured table (conv_tuning_table.h,
    // generated by tools/tune_splitk.py from in-network per-layer timings, kernel + reduce + launch gap); (2) for shapes
    // the table does not know, the rule distilled from it: split only grids of fewer than ~400 tiles, into about 448 / tiles
    // slices of at least 8 K-steps (two resident workgroups per CU; a cost model built from probe constants did worse
    // than this rule: 484.7 vs 494.9 frames/s).
    const int total_steps = conv_total_steps(a);
    const long blocks = (long)cdiv(a.M, 64) * cdiv(a.Cout, 64);
    const bool ring_path = a.rowrun || (a.in_scale_expected == 0 && a.up == 1 && a.Cin % 32 == 0);
    int s = tuning_lookup(a.M, a.Cout, a.K, a.KH, ring_path ? 1 : 0);
    const int thr = sw().split_below, target = sw().split_target;
    if (s > 0) {
        s = std::min(s, std::max(1, total_steps / 2));
    } else if (blocks < thr && a.Cout % 4 == 0) {
        s = (int)((target + blocks / 2) / blocks);
        s = std::min(s, std::max(1, total_steps / 8));
        s = std::min(s, 32);
    } else {
        s = 1;
    }
    splitk = std::max(1, s);
    return T64x64;
}

size_t conv_plan(ConvArgs& a) {
    a.xcd_swizzle = sw().xcd;
    a.M = a.N * a.Ho * a.Wo;
    a.K = a.rowrun ? a.KH * 32 * cdiv(a.KW * a.Cin, 32) : a.KH * a.KW * a.Cin;
    if (a.x_ld == 0) a.x_ld = a.Cin;
    if (a.res_ld == 0) a.res_ld = a.Cout;
    sn_fastdiv_make((unsigned)(a.Ho * a.Wo), a.div_hw_mul, a.div_hw_shift);
    sn_fastdiv_make((unsigned)a.Wo, a.div_w_mul, a.div_w_shift);
    int splitk = 1;
    (void)pick_tile(a, splitk);
    const int total_steps = conv_total_steps(a);
    a.steps_per_split = cdiv(total_steps, splitk);
    a.splitk = cdiv(total_steps, a.steps_per_split);
    return a.splitk > 1 ? (size_t)a.splitk * a.M * a.Cout * sizeof(float) : 0;
}

// ---- the route of a launch (conv.h) ------------------------------------------------------------------------------------
// The register-staged kernel's (NBUF, BF16) in operand mode `operand`.
// 1x1 launches over the large maps (block 1 at 720p: M = 57 600) are bandwidth / epilogue shaped: ONE LDS stage (18 KB, twice
// the resident workgroups) beats the double-buffered loop there (30.4 -> 28.8 us, 33.7 -> 32.2 us); below that it loses 0.3 us.
// The bf16-operand and split variants exist for the inference tile (64 x 64 x 32) only.
static void igemm_variant(const ConvArgs& a, int bm, int bn, int bk, int mode, int operand, int& nbuf_out, int& bf16_out) {
    const int nbuf = sw().nbuf;
    bf16_out = (bm == 64 && bn == 64 && bk == 32) ? operand : 0;
    const bool one_stage = nbuf == 1 || (nbuf == 0 && mode == 0 && bm == 64 && bn == 64 && a.M >= 32768);
    nbuf_out = (bf16_out != 1 && one_stage) ? 1 : 2;
}

// LDS-DMA ring kernel (conv_ring_kernel.h): no A-operand prologue, stride-free addressing, Cin % 32 == 0, 64x64 tile.
static bool ring_eligible(const ConvArgs& a, int tile, bool has_prologue, bool lowk_ring = false) {
    if (a.rowrun) return true;                              // the row-run A operand exists only in the ring kernel
    // two-step tiles (1x1, K = 64) with a plain epilogue are 2 us faster per launch on the register-staged kernel (more resident
    // workgroups to overlap the 16 KB epilogues: 33.4 vs 35.3 us at M = 57 600, N = 256); the merged shortcut|conv1 launch stays here
    // (lowk_ring: the training step's dgrad with a weight image -- there the packed split kernel is level with it, conv.h)
    if (!lowk_ring && sw().lowk_igemm && a.KH == 1 && a.KW == 1 && a.Cin == 64 && a.x_ld == a.Cin && a.out_floor == nullptr) return false;
    return sw().ring && tile == T64x64 && !has_prologue && a.up == 1 && a.Cin % 32 == 0 && !sw().bk16;
}

// The ring kernel's fragment prologue (conv_ring_kernel.h PRO): 1x1 / stride 1 convolutions whose input carries a BN + ReLU
// prologue; not on bf16 operands (mode 1).
// The PRO form fetches a step's scales AND shifts with one DMA instruction: the shifts are addressed as an unsigned 32-bit byte
// offset from the (running) scale pointer.  Callers of the public operators pass two independent pointers: a shift vector below
// the scales, or 4 GiB or more above them, must take the register-staged kernel (which dereferences both pointers).
static bool ring_pro_vectors_ok(const ConvArgs& a) {
    if (a.in_scale == nullptr || a.in_shift == nullptr) return true;
    const long d = (long)(a.in_shift - a.in_scale);                   // floats
    return d >= 0 && d < (1L << 30);
}
static bool ring_pro_geometry(const ConvArgs& a, int operand, bool has_prologue) {
    return sw().ring_pro && sw().ring && operand != 1 && !sw().bk16 && has_prologue && a.KH == 1 && a.KW == 1 && a.stride == 1 && a.pad == 0 &&
           a.up == 1 && a.Cin % 32 == 0 && !a.rowrun && a.x_ld == a.Cin;
}
// One K group (<0, B, 1, 1>) with the launch's pointers: its epilogue has no consumer BN (the training forward), and the kernel takes
// `out_floor` as the pair distance.  Measured: the 36 paired 1x1 launches of the 8 x 288 x 512 step 61.2 -> 55.9 us (76 -> 82.8 TF),
// 494.7 -> 502.2 pairs/s.  The inference conv1 layers (prologue AND consumer BN) were tried on it too: 25.7 us against 23.5 / 28.7 us
// on the register-staged kernel, the same 310 us per frame in sum -- they stay where they were.
static bool ring_pro_eligible(const ConvArgs& a, int operand) {
    return ring_pro_geometry(a, operand, a.in_scale != nullptr) && a.out_scale == nullptr && a.out_floor == nullptr && ring_pro_vectors_ok(a);
}

// Split-K inside the workgroup (conv_ring_kernel.h, "KG"): a launch strategy for a given split count.  Ring path: 3 groups x 48 KiB
// of ring = one 12-wave workgroup per CU; the slices must be equal (steps % 3 == 0).  Measured at 720p (rocprofv3 inside the graph
// replay, block-3 conv2, M = 3600, N = 256, K = 2304): 45.3 us against 45.8 us + a 4.9 us reduce launch.  The register-staged
// kernel's two-group form lost (30.8 vs 24.3 + 4.9 us) and was removed.
// Two groups with the fragment prologue (conv_ring_f32_kernel<0, 0, 2, 1>): the 1x1 layers that carry a BN + ReLU prologue AND
// split K in two (the block-3 conv1 layers of a 720p frame, K = 1024: register-staged kernel x 2 slices + slabs + a reduce launch
// before) as one 8-wave workgroup per tile.  No K groups on bf16 operands (mode 1).
static int conv_kgroups(const ConvArgs& a, int operand, bool ring, bool has_prologue) {
    if (!sw().kgroups || a.splitk < 2 || operand == 1) return 1;
    if (a.steps_per_split * a.splitk != conv_total_steps(a)) return 1;
    if (ring && a.splitk == 3 && !a.rowrun) return 3;
    if (sw().kgroups_pro && !ring && a.splitk == 2 && ring_pro_geometry(a, operand, has_prologue) && ring_pro_vectors_ok(a)) return 2;
    return 1;
}

// The patch-stationary kernel's forms (ConvRoute::patch_cfg - 1): patch PH x PW, row blocks per wave WR, register sets of B planes NS.
struct PatchForm { int ph, pw, wr, ns; };
// Two ship, both 8 x 8 pixels: with two column blocks (Cout <= 64) only WR = 1 keeps four waves busy, one 32 x 32 tile each; from four
// column blocks on WR = 2 gives every wave one B fragment for two row blocks.  Measured and dropped:
// 4 x 8 pixels, 16 x 16 pixels with WR = 4, five register sets.
static const PatchForm g_patch_forms[] = {{8, 8, 1, 3}, {8, 8, 2, 3}};
constexpr int SN_PATCH_FORMS = 2;
constexpr size_t SN_PATCH_LDS_MAX = 160 * 1024;
// The form for a launch, 0: its planes do not fit the LDS of a CU (256 channels and more).
static int patch_cfg(const ConvArgs& a) {
    auto fits = [&](int cfg) { return sn_patch_lds_bytes(g_patch_forms[cfg - 1].ph, g_patch_forms[cfg - 1].pw, a.Cin) <= SN_PATCH_LDS_MAX; };
    const int forced = sw().patch_cfg;
    if (forced >= 1 && forced <= SN_PATCH_FORMS) return fits(forced) ? forced : 0;
    const int cfg = a.Cout <= 64 ? 1 : 2;
    return fits(cfg) ? cfg : 0;
}

// The Profiler kind of a route -- the ONE place that numbers the kernels (prof.h); conv_prof_kind_name() is its inverse by construction.
static int route_prof_kind(const ConvRoute& r) {
    switch (r.family) {
        case CONV_IGEMM:      // + 18 for the one-stage (NBUF = 1), + 36 per BF16 (operand mode 1..3)
            return PK_KERNEL_CONV_BASE + r.mode * 6 + r.tile * 2 + (r.bk == 32 ? 1 : 0) + (r.nbuf == 1 ? 18 : 0) + 36 * r.operand;
        case CONV_PACKED: return PK_KERNEL_CONV_PACKED + (r.pro ? 3 : r.mode);
        case CONV_PACKED_KG2: return PK_KERNEL_CONV_PACKED + (r.pro ? 6 : 4 + r.mode);
        case CONV_ASTAT: return PK_KERNEL_CONV_ASTAT;
        case CONV_PATCH: return PK_KERNEL_CONV_PATCH + r.patch_cfg - 1;
        default: break;
    }
    // the read-time split modes (2 / 3) have kinds of their own (PK_KERNEL_CONV_SPLIT): their ring, K-group and PRO launches
    const int split = r.operand >= 2 ? PK_KERNEL_CONV_SPLIT + 8 * (r.operand - 2) : 0;
    if (r.family == CONV_RING) return split ? split + r.mode : PK_KERNEL_CONV_RING + r.mode + (r.operand ? 3 : 0);
    if (r.family == CONV_RING_PRO) return split ? split + 5 : PK_KERNEL_CONV_KG + 2;
    if (r.kg == 2) return split ? split + 6 : PK_KERNEL_CONV_KG + 3;
    return split ? split + 3 + r.mode : PK_KERNEL_CONV_KG + r.mode;
}

ConvRoute conv_route(const ConvArgs& a, int operand_mode, bool has_image, bool lowk_ring) {
    const ConvSwitches& s = sw();
    const bool image = operand_mode == 4 && has_image;
    const int op = operand_mode == 4 ? 0 : operand_mode;     // every kernel but the packed one runs mode 4 as exact f32
    int splitk_unused = 1;
    const int t = pick_tile(a, splitk_unused);
    const bool t64 = t == T64x64, bk32 = conv_bk(a) == 32;
    const bool has_pro = a.in_scale != nullptr;
    const bool ring = ring_eligible(a, t, has_pro, lowk_ring && image);
    const bool slabs = a.splitk == 1 || a.partial != nullptr;
    int kg = t64 ? conv_kgroups(a, op, ring, has_pro) : 1;
    // the packed split kernel has no three-way in-workgroup split-K (60 KiB of ring per group): a ring launch that would split K three
    // ways inside the workgroup goes through the slabs + reduce launch instead
    if (image && s.packed_kg3 && ring && kg == 3 && a.K % 32 == 0 && slabs) kg = 1;
    const bool pro = kg == 1 && !ring && t64 && bk32 && ring_pro_eligible(a, op);
    // packed split kernel with the fragment prologue: 1x1 / stride 1 layers that carry an input BN + ReLU (register-staged kernel or
    // the two-group PRO ring form otherwise); a K split goes through the slabs + reduce launch, or runs as two K groups (below)
    const bool packed_pro = image && s.packed_pro && !ring && t64 && bk32 && ring_pro_geometry(a, op, has_pro) &&
                            a.out_floor == nullptr /* the kernel's pair distance */ && ring_pro_vectors_ok(a) && slabs;
    if (packed_pro) kg = 1;
    const bool packed = (image && ring && kg == 1 && a.K % 32 == 0) || packed_pro;
    // a two-way K split with equal halves runs inside the packed workgroup (no slabs, no reduce launch)
    const bool packed_kg2 = packed && s.packed_kg2 && a.splitk == 2 && !a.rowrun && a.steps_per_split * 2 == conv_total_steps(a);
    if (packed_kg2) kg = 2;
    // A-stationary packed kernel: plain packed 1x1 launches (no prologue, no K split of any kind) over K <= 256 with many 32-column
    // blocks to reuse the split A tile on; the training step's dgrad (lowk_ring) keeps its kernels.  Smallest M (measured in the 720p
    // frame): with fewer M tiles than resident slots N is cut into groups, every group loads and
    // splits the A tile again, and a wave is left with one or two column blocks -- at M = 3600 that still pays for Cout x K = 1024 x
    // 256 (21.5 -> 20.4 us) and loses for 512 x 128 (12.1 -> 12.6 us), which wins at M = 14400 (26.5 -> 20.9 us).  The cut between
    // those two measured points is REASONED, not measured: 8192 rows = 256 M tiles = one per CU, from where on N is no longer cut
    // (the 1080p frame's 8160 x 512 x 128 launch falls 32 rows short of it and was never tried on this kernel); below 2048 the ring
    // kernel's N-parallel tiles fill the chip better in any case
    const int astat_min_m = s.astat_min_m > 0 ? s.astat_min_m : ((long)a.Cout * a.K >= 128 * 1024 ? 2048 : 8192);
    const bool astat = packed && !packed_pro && !packed_kg2 && kg == 1 && a.splitk == 1 && s.astat && !lowk_ring && !a.rowrun &&
                       a.KH == 1 && a.KW == 1 && a.stride == 1 && a.pad == 0 && a.up == 1 && a.K <= 256 && a.Cout >= s.astat_min_cout &&
                       a.M >= astat_min_m;
    // Patch-stationary packed kernel: packed 3x3 / pad 1 / stride 1 launches without a prologue and without slabs (no K split, or
    // the two equal K halves the ring kernel runs inside the workgroup: the kernel keeps that arithmetic; the stride-2 layers keep
    // the ring kernel) whose halo patch fits LDS; the training step's
    // dgrad (lowk_ring) keeps its kernels.  Smallest M: REASONED, not measured -- 12288 rows are 192 patches of 8 x 8
    // pixels, three workgroups per four CUs; below that the ring kernel's 64 x 64 tiles, cut in N as well, fill the chip better.  The
    // recorded small-shape routes (M <= 1224) and the 288 x 512 frame (M = 9216), whose launches tests count by kernel name, stay
    // what they are; the 360 x 640 frame's block 1 (M = 14400) moves
    const int patch_form = patch_cfg(a);
    const bool patch = packed && !packed_pro && ((kg == 1 && a.splitk == 1) || packed_kg2) && s.patch && !lowk_ring && !a.rowrun &&
                       a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1 && a.up == 1 && a.Cin % 32 == 0 && patch_form != 0 &&
                       a.M >= (s.patch_min_m > 0 ? s.patch_min_m : 12288);

    ConvRoute r{};
    r.tile = t;
    r.bk = bk32 ? 32 : 16;
    r.mode = (a.up > 1 || a.rowrun) ? 2 : (a.pad == 0 ? 0 : 1);
    r.operand = op;
    r.kg = kg;
    r.reduce = (a.splitk > 1 && kg == 1) ? 1 : 0;
    if (astat) {
        r.family = CONV_ASTAT;
        r.operand = 4;
        r.astat_bm = 32;                                     // (64 rows measured level at K = 128 and do not fit at K = 256: not built)
    } else if (patch) {
        r.family = CONV_PATCH;
        r.operand = 4;
        r.patch_cfg = patch_form;
    } else if (packed) {
        r.family = packed_kg2 ? CONV_PACKED_KG2 : CONV_PACKED;
        r.operand = 4;
        r.pro = packed_pro ? 1 : 0;
    } else if (pro) {
        r.family = CONV_RING_PRO;
        r.pro = 1;
    } else if (kg > 1) {
        r.family = CONV_RING_KG;
        r.pro = kg == 2 ? 1 : 0;                             // (two groups exist with the prologue only, three without it only)
    } else if (ring) {
        r.family = CONV_RING;
    } else {
        int bm, bn;
        tile_dims(t, bm, bn);
        r.family = CONV_IGEMM;
        igemm_variant(a, bm, bn, r.bk, r.mode, op, r.nbuf, r.operand);
    }
    r.prof_kind = route_prof_kind(r);
    return r;
}

const char* conv_prof_kind_name(int kind) {
    // every route the launchers take, named as rocprofv3 prints the template instantiation, at the kind route_prof_kind() gives it
    static const std::vector<std::string> names = [] {
        std::vector<std::string> v(PK_KERNEL_CONV_UNIT_PAIR + 4);
        char buf[96];
        auto ring = [&](int family, int mode, int operand, int kg, int pro) {
            ConvRoute r{};
            r.family = family; r.mode = mode; r.operand = operand; r.kg = kg; r.pro = pro;
            snprintf(buf, sizeof(buf), "conv_ring_f32_kernel<%d, %d, %d, %d>", mode, operand, kg, pro);
            v[route_prof_kind(r)] = buf;
        };
        for (int operand = 0; operand < 4; ++operand) {
            for (int mode = 0; mode < 3; ++mode) ring(CONV_RING, mode, operand, 1, 0);
            if (operand == 1) continue;
            ring(CONV_RING_KG, 0, operand, 3, 0); ring(CONV_RING_KG, 1, operand, 3, 0);
            ring(CONV_RING_PRO, 0, operand, 1, 1); ring(CONV_RING_KG, 0, operand, 2, 1);
        }
        for (int mode = 0; mode < 3; ++mode) ring(CONV_PACKED, mode, 4, 1, 0);
        ring(CONV_PACKED, 0, 4, 1, 1);
        ring(CONV_PACKED_KG2, 0, 4, 2, 0); ring(CONV_PACKED_KG2, 1, 4, 2, 0); ring(CONV_PACKED_KG2, 0, 4, 2, 1);
        {
            ConvRoute r{};
            r.family = CONV_ASTAT; r.astat_bm = 32;
            snprintf(buf, sizeof(buf), "conv_astat_f32_kernel<%d>", r.astat_bm);
            v[route_prof_kind(r)] = buf;
        }
        for (int cfg = 1; cfg <= SN_PATCH_FORMS; ++cfg) {
            ConvRoute r{};
            r.family = CONV_PATCH; r.patch_cfg = cfg;
            const PatchForm& f = g_patch_forms[cfg - 1];
            snprintf(buf, sizeof(buf), "conv_patch_f32_kernel<%d, %d, %d, %d>", f.ph, f.pw, f.wr, f.ns);
            v[route_prof_kind(r)] = buf;
        }
        for (int i = 0; i < 144; ++i) {                      // <BM, BN, BK, WM, WN, MODE, NBUF, BF16>
            ConvRoute r{};
            r.family = CONV_IGEMM;
            r.operand = i / 36; r.nbuf = 2 - i / 18 % 2; r.mode = i / 6 % 3; r.tile = i / 2 % 3; r.bk = (i & 1) ? 32 : 16;
            int bm, bn;
            tile_dims(r.tile, bm, bn);
            snprintf(buf, sizeof(buf), "conv_igemm_f32_kernel<%d, %d, %d, %d, %d, %d, %d, %d>", bm, bn, r.bk, bm / 2, bn / 2, r.mode, r.nbuf, r.operand);
            v[route_prof_kind(r)] = buf;
        }
        for (int i = 0; i < 4; ++i) {                        // conv_launch_pair: + 2 * MODE + (BK == 32)
            snprintf(buf, sizeof(buf), "conv_igemm_f32_pair_kernel<64, 64, %d, 32, 32, %d>", (i & 1) ? 32 : 16, i / 2);
            v[PK_KERNEL_CONV_PAIR + i] = buf;
        }
        v[PK_KERNEL_CONV_B2B] = "conv_b2b_f32_kernel<2>";
        v[PK_KERNEL_CONV_B2B + 1] = "conv_b2b_f32_kernel<4>";
        for (int i = 0; i < 4; ++i) {
            snprintf(buf, sizeof(buf), "conv_unit_pair_f32_kernel<%d, %d>", i >> 1, (i & 1) ? 64 : 32);
            v[PK_KERNEL_CONV_UNIT_PAIR + i] = buf;
        }
        return v;
    }();
    return (kind >= 0 && kind < (int)names.size() && !names[kind].empty()) ? names[kind].c_str() : nullptr;
}

// ---- the grid of a launch (conv.h conv_grid) ---------------------------------------------------------------------------
static int g_reserved_cus = 0;    // CUs the persistent grids leave to a communication stream (stabnet_conv_reserve_cus)
// persistent grids are sized for the CUs that are NOT reserved (never fewer than an eighth of the chip)
static int usable_cus(int cus) { return std::max(cus / 8, cus - std::max(0, g_reserved_cus)); }

// Register-staged kernel: one workgroup per (M tile, N tile, K slice).
static ConvGrid igemm_grid(const ConvArgs& a, int bm, int bn) {
    ConvGrid g{};
    g.gx = cdiv(a.M, bm); g.gy = cdiv(a.Cout, bn); g.gz = a.splitk;
    g.tiles = g.wgs = (long)g.gx * g.gy * g.gz;
    return g;
}
// Every ring launch.  The grid is persistent: at most the resident workgroups -- 3 per CU (48 KiB of LDS each), 2 of the packed
// split kernel (60 KiB), one when K splits inside the workgroup (KG x that; the K slices are then no tiles of their own).
static ConvGrid ring_grid(const ConvRoute& r, const ConvArgs& a, int cus) {
    ConvGrid g{};
    const int per_cu = r.kg > 1 ? 1 : (r.operand == 4 ? sw().packed_wgs_per_cu : sw().ring_wgs_per_cu);
    g.tiles = (long)cdiv(a.M, 64) * cdiv(a.Cout, 64) * (r.kg > 1 ? 1 : a.splitk);
    g.gx = (int)std::min<long>(g.tiles, (long)per_cu * usable_cus(cus));
    g.gy = g.gz = 1;
    g.wgs = g.gx;
    return g;
}
// The A-stationary packed kernel: grid = (M tiles, N groups).  A group is a multiple of four 32-column blocks (one per wave and pass);
// N is cut into groups only as far as it takes to fill the resident slots (two workgroups of 64 KB of LDS per CU): every further
// group splits the A tile once more.  Tiles: (M tile, pass of four column blocks).
static ConvGrid astat_grid(const ConvArgs& a, int bm, int cus) {
    ConvGrid g{};
    const int mtiles = cdiv(a.M, bm), nblk = 2 * cdiv(a.Cout, 64);
    int groups = (int)std::min<long>(cdiv(nblk, 4), std::max<long>(1, 2L * usable_cus(cus) / mtiles));
    groups = cdiv(nblk, 4 * cdiv(cdiv(nblk, groups), 4));            // as the kernel derives the group size from it: no empty group
    g.gx = mtiles; g.gy = groups; g.gz = 1;
    g.tiles = (long)mtiles * cdiv(nblk, 4);
    g.wgs = (long)mtiles * groups;
    return g;
}
// The patch-stationary packed kernel: grid = (patches, N groups).  A group is a multiple of the CS column blocks the workgroup's waves
// work on side by side; N is cut into groups only as far as it takes to fill the resident slots: every further group loads and splits
// the patch once more.  Tiles: (patch, pass of CS column blocks).
static ConvGrid patch_grid(const ConvArgs& a, int ph, int pw, int wr, int cus) {
    ConvGrid g{};
    const size_t lds = sn_patch_lds_bytes(ph, pw, a.Cin);
    const int cs = 4 / ((ph / 4) * (pw / 8) / wr);
    const int mtiles = a.N * cdiv(a.Ho, ph) * cdiv(a.Wo, pw), nblk = 2 * cdiv(a.Cout, 64);
    const long slots = (long)std::min<size_t>(wr >= 4 ? 1 : 2, SN_PATCH_LDS_MAX / lds) * usable_cus(cus);
    int groups = (int)std::min<long>(cdiv(nblk, cs), std::max<long>(1, slots / mtiles));
    groups = cdiv(nblk, cs * cdiv(cdiv(nblk, groups), cs));          // as the kernel derives the group size from it: no empty group
    g.gx = mtiles; g.gy = groups; g.gz = 1;
    g.tiles = (long)mtiles * cdiv(nblk, cs);
    g.wgs = (long)mtiles * groups;
    return g;
}
ConvGrid conv_grid(const ConvRoute& r, const ConvArgs& a, int cus) {
    switch (r.family) {
        case CONV_IGEMM: {
            int bm, bn;
            tile_dims(r.tile, bm, bn);
            return igemm_grid(a, bm, bn);
        }
        case CONV_ASTAT: return astat_grid(a, r.astat_bm, cus);
        case CONV_PATCH: {
            if (r.patch_cfg < 1 || r.patch_cfg > SN_PATCH_FORMS) return ConvGrid{};
            const PatchForm& f = g_patch_forms[r.patch_cfg - 1];
            return patch_grid(a, f.ph, f.pw, f.wr, cus);
        }
        default: return ring_grid(r, a, cus);
    }
}
size_t conv_astat_plane_bytes(const ConvRoute& r, const ConvArgs& a) { return (size_t)r.astat_bm * a.K * 6; }
size_t conv_astat_plane_limit() { return (size_t)SN_ASTAT_A_BYTES; }
size_t conv_patch_lds_bytes(const ConvRoute& r, const ConvArgs& a) {
    if (r.patch_cfg < 1 || r.patch_cfg > SN_PATCH_FORMS) return 0;
    return sn_patch_lds_bytes(g_patch_forms[r.patch_cfg - 1].ph, g_patch_forms[r.patch_cfg - 1].pw, a.Cin);
}
size_t conv_patch_lds_limit() { return SN_PATCH_LDS_MAX; }
int conv_plan_total_steps(const ConvArgs& a) { return conv_total_steps(a); }

// ---- launchers ---------------------------------------------------------------------------------------------------------
// Dynamic LDS above what `kern` is set up for: a launch that needs `need` bytes opts the kernel in to `limit` bytes first.  `configured`
// is the caller's record, one per kernel instantiation, of the size set up so far (64 KB need no opt-in).
static int lds_opt_in(const void* kern, size_t need, size_t limit, size_t& configured, const char* who) {
    if (need <= configured) return STABNET_OK;
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit);
    if (e != hipSuccess) {
        stabnet_set_error("%s: hipFuncSetAttribute(%zu B LDS) failed: %s", who, limit, hipGetErrorString(e));
        return STABNET_ERR_LAUNCH;
    }
    configured = limit;
    return STABNET_OK;
}

template <int BM, int BN, int BK, int WM, int WN, int MODE, int NBUF, int BF16 = 0>
static int launch_one_nb(const ConvArgs& a, hipStream_t st) {
    constexpr size_t lds_op = NBUF * (size_t)(BM + BN) * (BK + 4) * sizeof(float);
    constexpr size_t lds_epi = 4 * (size_t)SN_EPI_WAVE_BYTES;        // the epilogue's transposition scratch
    constexpr size_t lds = lds_op > lds_epi ? lds_op : lds_epi;
    static size_t configured = 64 * 1024;
    auto kern = conv_igemm_f32_kernel<BM, BN, BK, WM, WN, MODE, NBUF, BF16>;
    if (const int rc = lds_opt_in(reinterpret_cast<const void*>(kern), lds, lds, configured, "conv")) return rc;
    const ConvGrid g = igemm_grid(a, BM, BN);
    kern<<<dim3(g.gx, g.gy, g.gz), 256, lds, st>>>(a);
    SN_LAUNCH_CHECK("conv_igemm_f32_kernel");
    return STABNET_OK;
}

template <int BM, int BN, int BK, int WM, int WN, int MODE>
static int launch_one_t(const ConvRoute& r, const ConvArgs& a, hipStream_t st) {
    if constexpr (BM == 64 && BN == 64 && BK == 32) {
        if (r.operand == 1) return launch_one_nb<BM, BN, BK, WM, WN, MODE, 2, 1>(a, st);
        else if (r.operand == 2) return r.nbuf == 1 ? launch_one_nb<BM, BN, BK, WM, WN, MODE, 1, 2>(a, st) : launch_one_nb<BM, BN, BK, WM, WN, MODE, 2, 2>(a, st);
        else if (r.operand == 3) return r.nbuf == 1 ? launch_one_nb<BM, BN, BK, WM, WN, MODE, 1, 3>(a, st) : launch_one_nb<BM, BN, BK, WM, WN, MODE, 2, 3>(a, st);
    }
    return r.nbuf == 1 ? launch_one_nb<BM, BN, BK, WM, WN, MODE, 1>(a, st) : launch_one_nb<BM, BN, BK, WM, WN, MODE, 2>(a, st);
}

template <int BM, int BN, int BK, int WM, int WN>
static int launch_one(const ConvRoute& r, const ConvArgs& a, hipStream_t st) {
    if (r.mode == 2) return launch_one_t<BM, BN, BK, WM, WN, 2>(r, a, st);
    if (r.mode == 0) return launch_one_t<BM, BN, BK, WM, WN, 0>(r, a, st);
    return launch_one_t<BM, BN, BK, WM, WN, 1>(r, a, st);
}

static int launch_igemm(const ConvRoute& r, const ConvArgs& a, hipStream_t st) {
    if (r.bk == 32) {
        if (r.tile == T128x128) return launch_one<128, 128, 32, 64, 64>(r, a, st);
        if (r.tile == T128x64) return launch_one<128, 64, 32, 64, 32>(r, a, st);
        return launch_one<64, 64, 32, 32, 32>(r, a, st);
    }
    if (r.tile == T128x128) return launch_one<128, 128, 16, 64, 64>(r, a, st);
    if (r.tile == T128x64) return launch_one<128, 64, 16, 64, 32>(r, a, st);
    return launch_one<64, 64, 16, 32, 32>(r, a, st);
}

// CUs of the current device (read once per process)
static int device_cus(int& cus) {
    static int cached = 0;
    if (cached == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
            stabnet_set_error("conv: cannot read the CU count");
            return STABNET_ERR_LAUNCH;
        }
        cached = n;
    }
    cus = cached;
    return STABNET_OK;
}
static thread_local int g_last_launch_kind = -1;   // stabnet_conv_last_launch_kind

// The ONE mapping from a route's (MODE, operand, KG, PRO) to the instantiation of conv_ring_f32_kernel (256 threads per K group);
// false: the library has no such kernel.
template <int B>
static bool launch_ring_operand(const ConvRoute& r, const ConvArgs& a, int grid, hipStream_t st) {
    const int key = 100 * r.mode + 10 * r.kg + r.pro;
    if (key == 10) { conv_ring_f32_kernel<0, B><<<grid, 256, 0, st>>>(a); return true; }
    if (key == 110) { conv_ring_f32_kernel<1, B><<<grid, 256, 0, st>>>(a); return true; }
    if (key == 210) { conv_ring_f32_kernel<2, B><<<grid, 256, 0, st>>>(a); return true; }
    if constexpr (B != 1) {                                  // the fragment prologue: one / two K groups
        if (key == 11) { conv_ring_f32_kernel<0, B, 1, 1><<<grid, 256, 0, st>>>(a); return true; }
        if (key == 21) { conv_ring_f32_kernel<0, B, 2, 1><<<grid, 512, 0, st>>>(a); return true; }
    }
    if constexpr (B == 0 || B == 2 || B == 3) {              // three K groups
        if (key == 30) { conv_ring_f32_kernel<0, B, 3><<<grid, 768, 0, st>>>(a); return true; }
        if (key == 130) { conv_ring_f32_kernel<1, B, 3><<<grid, 768, 0, st>>>(a); return true; }
    }
    if constexpr (B == 4) {                                  // the packed split kernel's two K groups
        if (key == 20) { conv_ring_f32_kernel<0, B, 2, 0><<<grid, 512, 0, st>>>(a); return true; }
        if (key == 120) { conv_ring_f32_kernel<1, B, 2, 0><<<grid, 512, 0, st>>>(a); return true; }
    }
    return false;
}

// Every ring launch, on ring_grid()'s persistent grid.
static int launch_ring_route(const ConvRoute& r, const ConvArgs& a, hipStream_t st) {
    int cus = 0;
    if (const int rc = device_cus(cus)) return rc;
    const int grid = ring_grid(r, a, cus).gx;
    bool ok = false;
    switch (r.operand) {
        case 0: ok = launch_ring_operand<0>(r, a, grid, st); break;
        case 1: ok = launch_ring_operand<1>(r, a, grid, st); break;
        case 2: ok = launch_ring_operand<2>(r, a, grid, st); break;
        case 3: ok = launch_ring_operand<3>(r, a, grid, st); break;
        case 4: ok = launch_ring_operand<4>(r, a, grid, st); break;
        default: break;
    }
    SN_REQUIRE(ok, "conv: no conv_ring_f32_kernel<%d, %d, %d, %d>", r.mode, r.operand, r.kg, r.pro);
    SN_LAUNCH_CHECK("conv_ring_f32_kernel");
    return STABNET_OK;
}

// The A-stationary packed kernel, on astat_grid()'s (M tiles, N groups).
static int launch_astat(const ConvRoute& r, const ConvArgs& a, hipStream_t st) {
    int cus = 0;
    if (const int rc = device_cus(cus)) return rc;
    const int bm = r.astat_bm;
    SN_REQUIRE(bm == 32 && a.K % 32 == 0 && (size_t)bm * a.K * 6 <= (size_t)SN_ASTAT_A_BYTES && a.splitk == 1,
               "conv: the A-stationary kernel takes BM %d x K %d without a K split only if the planes fit %d bytes", bm, a.K, SN_ASTAT_A_BYTES);
    const ConvGrid g = astat_grid(a, bm, cus);
    const dim3 grid(g.gx, g.gy);
    conv_astat_f32_kernel<32><<<grid, 256, 0, st>>>(a);
    SN_LAUNCH_CHECK("conv_astat_f32_kernel");
    return STABNET_OK;
}

// The patch-stationary packed kernel, on patch_grid()'s (patches, N groups).
template <int PH, int PW, int WR, int NS>
static int launch_patch_one(const ConvArgs& a, int cus, hipStream_t st) {
    const size_t lds = sn_patch_lds_bytes(PH, PW, a.Cin);
    auto kern = conv_patch_f32_kernel<PH, PW, WR, NS>;
    static size_t configured = 64 * 1024;
    if (const int rc = lds_opt_in(reinterpret_cast<const void*>(kern), lds, SN_PATCH_LDS_MAX, configured, "conv")) return rc;
    const ConvGrid g = patch_grid(a, PH, PW, WR, cus);
    const dim3 grid(g.gx, g.gy);
    kern<<<grid, 256, lds, st>>>(a);
    SN_LAUNCH_CHECK("conv_patch_f32_kernel");
    return STABNET_OK;
}
static int launch_patch(const ConvRoute& r, const ConvArgs& a, hipStream_t st) {
    int cus = 0;
    if (const int rc = device_cus(cus)) return rc;
    SN_REQUIRE(a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1 && a.up == 1 && a.Cin % 32 == 0 &&
                   (a.splitk == 1 || (a.splitk == 2 && a.steps_per_split * 2 == conv_total_steps(a))) && a.Ho == a.H && a.Wo == a.W && r.patch_cfg >= 1 &&
                   r.patch_cfg <= SN_PATCH_FORMS &&
                   sn_patch_lds_bytes(g_patch_forms[r.patch_cfg - 1].ph, g_patch_forms[r.patch_cfg - 1].pw, a.Cin) <= SN_PATCH_LDS_MAX,
               "conv: the patch-stationary kernel takes 3x3 / pad 1 / stride 1 over Cin %d (a multiple of 32) without a K split or with two equal K halves only if the planes fit %zu bytes",
               a.Cin, SN_PATCH_LDS_MAX);
    return r.patch_cfg == 1 ? launch_patch_one<8, 8, 1, 3>(a, cus, st) : launch_patch_one<8, 8, 2, 3>(a, cus, st);
}

// ---- pre-split weight image (conv.h) -----------------------------------------------------------------------------------
size_t conv_weight_image_floats(int Cout, int K) { return (size_t)cdiv(Cout, 64) * (size_t)(K / 32) * 3072; }

// sn_split3 with a saturating head: a finite |w| >= 2^127 (2 - 2^-8) rounds to a bf16 infinity (h = inf, m = -inf, l = NaN for
// FLT_MAX); its head is the largest finite bf16 (0x7F7F) instead, and h + m + l == w stays exact (FLT_MAX = (2^128 - 2^120) + 2^120
// - 2^104).  Fold time only (the weight image); infinities and NaN keep h = w.
__device__ __forceinline__ unsigned weight_split_head(float& x0, float& x1) {
    const float top = __builtin_bit_cast(float, 0x7F7F0000u), fmax = __builtin_bit_cast(float, 0x7F7FFFFFu);
    const float h0 = (fabsf(x0) > top && fabsf(x0) <= fmax) ? copysignf(top, x0) : x0;
    const float h1 = (fabsf(x1) > top && fabsf(x1) <= fmax) ? copysignf(top, x1) : x1;
    const unsigned p = sn_pack_bf16(h0, h1);
    x0 = sn_sub_f32(x0, __builtin_bit_cast(float, p << 16));
    x1 = sn_sub_f32(x1, __builtin_bit_cast(float, p & 0xffff0000u));
    return p;
}
__device__ __forceinline__ SnSplit3 weight_split3(const f32x4 x) {
    float a = x.x, b = x.y, c = x.z, d = x.w;
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    u32x2 h, m, l;
    h.x = weight_split_head(a, b); h.y = weight_split_head(c, d);
    m.x = sn_split_level(a, b); m.y = sn_split_level(c, d);
    l.x = sn_pack_bf16(a, b); l.y = sn_pack_bf16(c, d);
    SnSplit3 s;
    s.h = __builtin_bit_cast(sn_bf16x4, h); s.m = __builtin_bit_cast(sn_bf16x4, m); s.l = __builtin_bit_cast(sn_bf16x4, l);
    return s;
}

// one thread per (N tile, K step, wave column, k group, lane): 8 weights -> three 16-byte plane entries
__device__ __forceinline__ void weight_split_image_thread(const float* __restrict__ w, int Cout, int K, uint4* __restrict__ img, long i) {
    const int steps = K / 32;
    const int lane = (int)(i & 63), j = (int)((i >> 6) & 1), wn = (int)((i >> 7) & 1);
    const long ts = i >> 8;                                  // nt * steps + ks
    const int ks = (int)(ts % steps), nt = (int)(ts / steps);
    const int n = nt * 64 + wn * 32 + (lane & 31), g = lane >> 5;
    f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
    if (n < Cout) {
        const float* r = w + (size_t)n * K + ks * 32 + 16 * j + 4 * g;
        lo = *reinterpret_cast<const f32x4*>(r);
        hi = *reinterpret_cast<const f32x4*>(r + 8);
    }
    const SnSplit3 a = weight_split3(lo), b = weight_split3(hi);
    uint4* out = img + ts * 768 + (size_t)(wn * 6 + j) * 64 + lane;       // 16-byte units: stage 768, chunk 64
    out[0] = __builtin_bit_cast(uint4, SN_CAT8(a.h, b.h));
    out[2 * 64] = __builtin_bit_cast(uint4, SN_CAT8(a.m, b.m));
    out[4 * 64] = __builtin_bit_cast(uint4, SN_CAT8(a.l, b.l));
}

__global__ __launch_bounds__(256) void weight_split_image_kernel(const float* __restrict__ w, int Cout, int K, uint4* __restrict__ img) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)((Cout + 63) / 64) * (K / 32) * 256) return;
    weight_split_image_thread(w, Cout, K, img, i);
}

__global__ __launch_bounds__(256) void weight_split_images_kernel(const float* __restrict__ w_base, float* __restrict__ img_base, const WeightImageTable t) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= t.tprefix[t.n]) return;
    int e = 0;
    while (i >= t.tprefix[e + 1]) ++e;                       // (every matrix covers whole 256-thread blocks: uniform per block)
    weight_split_image_thread(w_base + t.w_off[e], t.Cout[e], t.K[e], reinterpret_cast<uint4*>(img_base + t.img_off[e]), i - t.tprefix[e]);
}

void weight_image_table_add(WeightImageTable& t, long w_off, long img_off, int Cout, int K) {
    if (t.n == 0) t.tprefix[0] = 0;
    t.w_off[t.n] = w_off; t.img_off[t.n] = img_off; t.Cout[t.n] = Cout; t.K[t.n] = K;
    t.tprefix[t.n + 1] = t.tprefix[t.n] + (long)cdiv(Cout, 64) * (K / 32) * 256;
    ++t.n;
}

int launch_weight_split_images(const float* w_base, float* img_base, const WeightImageTable& t, hipStream_t st) {
    if (t.n == 0) return STABNET_OK;
    SN_REQUIRE(w_base && img_base && t.n <= 64, "weight images: bad table");
    weight_split_images_kernel<<<(unsigned)(t.tprefix[t.n] >> 8), 256, 0, st>>>(w_base, img_base, t);
    SN_LAUNCH_CHECK("weight_split_images_kernel");
    return STABNET_OK;
}

int launch_weight_split_image(const float* w, int Cout, int K, float* img, hipStream_t st) {
    SN_REQUIRE(w && img && Cout > 0 && K > 0 && K % 32 == 0, "weight image: K=%d must be a multiple of 32", K);
    const long total = (long)cdiv(Cout, 64) * (K / 32) * 256;
    weight_split_image_kernel<<<cdiv(total, 256), 256, 0, st>>>(w, Cout, K, reinterpret_cast<uint4*>(img));
    SN_LAUNCH_CHECK("weight_split_image_kernel");
    return STABNET_OK;
}

int conv_launch(const ConvArgs& a, hipStream_t st, Prof* prof, int bf16_operands, const float* w_img, bool lowk_ring) {
    SN_REQUIRE(a.rowrun || a.Cin % 16 == 0, "conv: Cin=%d must be a multiple of 16 (pad the channels)", a.Cin);
    SN_REQUIRE(!a.rowrun || (a.in_scale == nullptr && a.up == 1 && a.KH <= 8 && cdiv(a.KW * a.Cin, 32) <= 4),
               "conv: row-run operand needs no prologue, KH <= 8 and KW*Cin <= 128");
    SN_REQUIRE(a.Cout % 4 == 0, "conv: Cout=%d must be a multiple of 4", a.Cout);
    SN_REQUIRE(a.splitk >= 1 && a.steps_per_split >= 1 && a.div_hw_mul != 0, "conv: conv_plan() not called");
    SN_REQUIRE(a.splitk == 1 || a.partial != nullptr, "conv: split-K needs a workspace");
    const ConvRoute r = conv_route(a, bf16_operands, w_img != nullptr, lowk_ring);
    SN_REQUIRE(r.family != CONV_IGEMM || a.x_ld == a.Cin, "conv: a strided input (x_ld %d != Cin %d) needs the ring kernel", a.x_ld, a.Cin);
    g_last_launch_kind = r.prof_kind;
    const bool rec = prof != nullptr && prof->begin(st);
    int rc;
    switch (r.family) {
        case CONV_IGEMM: rc = launch_igemm(r, a, st); break;
        case CONV_PACKED:
        case CONV_PACKED_KG2: {
            ConvArgs b = a;
            b.w = w_img;
            rc = launch_ring_route(r, b, st);
            break;
        }
        case CONV_ASTAT: {
            ConvArgs b = a;
            b.w = w_img;
            rc = launch_astat(r, b, st);
            break;
        }
        case CONV_PATCH: {
            ConvArgs b = a;
            b.w = w_img;
            rc = launch_patch(r, b, st);
            break;
        }
        default: rc = launch_ring_route(r, a, st); break;
    }
    if (rec) prof->end(st, r.prof_kind, 2.0 * a.M * (double)(a.KH * a.KW * (a.cin_real ? a.cin_real : a.Cin)) * a.Cout,
                       // algorithmic bytes: input + weights + output (or the split-K slabs) + the residual read
                       4.0 * ((double)a.N * a.H * a.W * a.Cin + (double)a.K * a.Cout + (double)a.M * a.Cout * (r.reduce ? a.splitk : 1) +
                              ((a.residual != nullptr && !r.reduce) ? (double)a.M * a.Cout : 0.0)),
                       a.M, a.Cout, a.K, a.splitk);
    if (rc) return rc;
    if (r.reduce) {
        const size_t q = (size_t)a.M * (a.Cout / 4);
        const bool rec2 = prof != nullptr && prof->begin(st);
        conv_splitk_reduce_kernel<<<cdiv((long)q, 256), 256, 0, st>>>(a);
        if (rec2) prof->end(st, PK_KERNEL_SPLITK_REDUCE, 0.0, 4.0 * (double)a.M * a.Cout * (a.splitk + 1 + (a.residual != nullptr ? 1 : 0)));
        SN_LAUNCH_CHECK("conv_splitk_reduce_kernel");
    }
    return STABNET_OK;
}

// The siamese pair as one launch (ConvPair, conv.h): the 64x64 register-staged tile, MODE 0 / 1, BK 32 or 16.
bool conv_pair_supported(const ConvArgs& a) {
    int splitk_unused = 1;
    const int t = pick_tile(a, splitk_unused);
    const bool pro = a.in_scale != nullptr || a.in_scale_expected;     // (at plan time the prologue pointers are not bound yet)
    return t == T64x64 && !ring_eligible(a, t, pro) && a.up == 1 && !a.rowrun && (a.x_ld == 0 || a.x_ld == a.Cin);
}

template <int BK, int MODE>
static int launch_pair_one(const ConvArgs& a, const ConvPair& pr, hipStream_t st) {
    constexpr size_t lds = 2 * (size_t)(64 + 64) * (BK + 4) * sizeof(float);
    static_assert(lds >= 4 * (size_t)SN_EPI_WAVE_BYTES && lds <= 64 * 1024, "LDS of the 64x64 tile");
    dim3 grid(cdiv(a.M, 64), cdiv(a.Cout, 64), a.splitk);
    conv_igemm_f32_pair_kernel<64, 64, BK, 32, 32, MODE><<<grid, 256, lds, st>>>(a, pr);
    SN_LAUNCH_CHECK("conv_igemm_f32_pair_kernel");
    return STABNET_OK;
}

int conv_launch_pair(const ConvArgs& a, const ConvPair& pr, hipStream_t st, Prof* prof, const float* w_img) {
    SN_REQUIRE(a.Cin % 16 == 0 && a.Cout % 4 == 0, "conv pair: Cin %% 16 and Cout %% 4 must be 0");
    SN_REQUIRE(a.splitk >= 1 && a.steps_per_split >= 1 && a.div_hw_mul != 0, "conv pair: conv_plan() not called");
    SN_REQUIRE(a.splitk == 1 || a.partial != nullptr, "conv pair: split-K needs a workspace");
    SN_REQUIRE(conv_pair_supported(a), "conv pair: the plan of this shape is not the 64x64 register-staged launch");
    SN_REQUIRE(pr.m_tower > 0 && pr.m_tower % 64 == 0 && a.M == 2 * pr.m_tower, "conv pair: tower rows %d must be a multiple of 64 (M %d)",
               pr.m_tower, a.M);
    const bool bk32 = conv_bk(a) == 32;
    const int mode = a.pad == 0 ? 0 : 1;
    // 1x1 layers: the LDS-DMA ring kernel with the BN + ReLU prologue on the A fragments, exact f32 (both towers in one launch: the
    // offsets of the second tower all derive from the distance of the two workspaces, which must be what ConvPair describes); with a
    // weight image the packed split kernel's prologue form
    const bool pro = bk32 && ring_pro_eligible(a, 0) && pr.dx == pr.dscale - (long)pr.m_tower * a.Cin && pr.dy == pr.dscale - (long)pr.m_tower * a.Cout &&
                     (a.residual == nullptr || pr.dres == pr.dscale - (long)(a.N / 2) * a.res_H * a.res_W * a.res_ld);
    const bool packed = pro && w_img != nullptr && a.K % 32 == 0 && a.splitk == 1;
    ConvRoute r{};
    r.family = packed ? CONV_PACKED : CONV_RING_PRO;
    r.operand = packed ? 4 : 0;
    r.kg = r.pro = 1;
    g_last_launch_kind = pro ? route_prof_kind(r) : PK_KERNEL_CONV_PAIR + mode * 2 + (bk32 ? 1 : 0);
    const bool rec = prof != nullptr && prof->begin(st);
    int rc;
    if (pro) {
        ConvArgs b = a;
        b.out_floor = reinterpret_cast<const float*>((size_t)pr.dscale);      // the kernel's pair distance (not a pointer: see conv_ring_kernel.h PRO)
        if (packed) b.w = w_img;
        rc = launch_ring_route(r, b, st);
    } else if (bk32) {
        rc = mode == 0 ? launch_pair_one<32, 0>(a, pr, st) : launch_pair_one<32, 1>(a, pr, st);
    } else {
        rc = mode == 0 ? launch_pair_one<16, 0>(a, pr, st) : launch_pair_one<16, 1>(a, pr, st);
    }
    if (rec) prof->end(st, pro ? route_prof_kind(r) : PK_KERNEL_CONV_PAIR + mode * 2 + (bk32 ? 1 : 0), 2.0 * a.M * (double)(a.KH * a.KW * (a.cin_real ? a.cin_real : a.Cin)) * a.Cout,
                       4.0 * ((double)a.N * a.H * a.W * a.Cin + (double)a.K * a.Cout + (double)a.M * a.Cout * a.splitk),
                       a.M, a.Cout, a.K, a.splitk);
    if (rc) return rc;
    if (a.splitk > 1) {
        const size_t q = (size_t)a.M * (a.Cout / 4);
        const bool rec2 = prof != nullptr && prof->begin(st);
        conv_splitk_reduce_pair_kernel<<<cdiv((long)q, 256), 256, 0, st>>>(a, pr);
        if (rec2) prof->end(st, PK_KERNEL_SPLITK_REDUCE, 0.0, 4.0 * (double)a.M * a.Cout * (a.splitk + 1));
        SN_LAUNCH_CHECK("conv_splitk_reduce_pair_kernel");
    }
    return STABNET_OK;
}

// ---- conv2 (3x3) -> conv3 (1x1) back to back (conv_b2b_kernel.h) ------------------------------------------
bool conv_b2b_supported(const ConvArgs& c2, const ConvArgs& c3) {
    // A LAUNCH strategy the inference plan does not choose by default (STABNET_CONV_B2B_PLAN=1 turns it on, net.hip): measured
    // in the 720p frame it loses to the two launches at every unit it applies to.  The operator
    // itself (stabnet_conv3x3_conv1x1_fwd) is always available.
    const bool g2 = c2.KH == 3 && c2.KW == 3 && c2.pad == 1 && c2.up == 1 && !c2.rowrun && (c2.stride == 1 || c2.stride == 2) &&
                    c2.Cin == c2.Cout && (c2.Cout == 64 || c2.Cout == 128) && c2.in_scale_expected == 0 && c2.in_scale == nullptr;
    const bool g3 = c3.KH == 1 && c3.KW == 1 && c3.pad == 0 && c3.stride == 1 && c3.up == 1 && !c3.rowrun && c3.Cin == c2.Cout &&
                    (c3.x_ld == 0 || c3.x_ld == c3.Cin) && c3.Cout % c2.Cout == 0 && c3.N == c2.N && c3.H == c2.Ho && c3.W == c2.Wo &&
                    c3.in_scale_expected == 0 && c3.in_scale == nullptr;
    return sw().b2b && sw().ring && g2 && g3;
}

int conv_b2b_launch(const ConvArgs& c2, const ConvArgs& c3, hipStream_t st, Prof* prof) {
    SN_REQUIRE(conv_b2b_supported(c2, c3), "conv b2b: unsupported geometry");
    SN_REQUIRE(c2.div_hw_mul != 0 && c3.div_hw_mul != 0 && c2.M == c3.M, "conv b2b: conv_plan() not called on both convolutions");
    SN_REQUIRE(c2.x && c2.w && c3.w && c3.y && c2.out_scale && c2.out_shift, "conv b2b: null pointer");
    SN_REQUIRE(c2.bias == nullptr && c2.residual == nullptr, "conv b2b: the 3x3 convolution takes no bias / residual");
    int cus = 0;
    if (const int rc = device_cus(cus)) return rc;
    B2bArgs P;
    P.c2 = c2;
    P.c3 = c3;
    P.c3.splitk = 1;                                                  // the accumulators handed to the epilogue are the full sum
    P.c3.steps_per_split = conv_total_steps(c3);
    const int tiles_m = cdiv(c2.M, 64);
    g_last_launch_kind = PK_KERNEL_CONV_B2B + (c2.Cout == 128 ? 1 : 0);
    const bool rec = prof != nullptr && prof->begin(st);
    if (c2.Cout == 64) {
        conv_b2b_f32_kernel<2><<<std::min(tiles_m, sw().b2b_wgs_per_cu * usable_cus(cus)), 256, 0, st>>>(P);
    } else {
        conv_b2b_f32_kernel<4><<<std::min(tiles_m, usable_cus(cus)), 512, 0, st>>>(P);    // 136 KB of LDS
    }
    if (rec) prof->end(st, PK_KERNEL_CONV_B2B + (c2.Cout == 128 ? 1 : 0),
                       2.0 * c2.M * ((double)c2.K * c2.Cout + (double)c3.K * c3.Cout),
                       4.0 * ((double)c2.N * c2.H * c2.W * c2.Cin + (double)c2.K * c2.Cout + (double)c3.K * c3.Cout +
                              (double)c3.M * c3.Cout * (c3.residual ? 2 : 1)),
                       c2.M, c3.Cout, c2.K + c3.K, 1);
    SN_LAUNCH_CHECK("conv_b2b_f32_kernel");
    return STABNET_OK;
}

// ---- conv3 -> next unit's conv1 as one launch (conv_pair_kernel.h) -------------------------------------------
// A property a plan gets when asked (stabnet_net_fuse_unit_pairs, net.hip): conv_route() and the default plans do not know it.
// Rule: both pair shapes of the network stay fused, by measurement (one visit, layer tables of the plan as built and of the fused plan,
// profiles/r23_layers_*): the fused row beats the sum of its two rows at every size taken --
//   f32 form <1, 64>   (64 -> 256 + residual, 256 -> 64)    720p, M = 57 600: 32.3 + 27.4 -> 53.7 us;  1080p, M = 129 600: 66.6 + 51.9 -> 107.0 us;
//                                                            360 x 640, M = 14 400: 13.8 + 14.3 -> 20.5 us
//   packed form <0, 32> (128 -> 512 + residual, 512 -> 128)  720p, M = 14 400: 21.3 + 22.9 -> 38.4 us; 1080p, M = 32 400: 42.0 + 40.8 -> 66.4 us
// (the other two instantiations, <1, 32> and <0, 64>, are the same code for 64 -> N1 -> 128 and 128 -> N1 -> 64 channels: no plan of the
// network has such a pair; the operator entry and its tests reach them).  Passes of 64 channels with the 64-row tile (half the chunk, three
// workgroups per CU) were measured and dropped: 57.8 - 58.5 us against 55.5 - 56.1 us.
constexpr size_t SN_PAIR_LDS_MAX = 96 * 1024;                 // the network's pairs take 48 / 64 KB (three / two workgroups per CU); K = 128 with 64-row tiles 96 KB
size_t conv_unit_pair_lds_limit() { return SN_PAIR_LDS_MAX; }

bool conv_unit_pair_form(const ConvArgs& c3, const ConvArgs& c1, bool img3, bool img1, ConvUnitPairForm& f) {
    f = ConvUnitPairForm{};
    if (!sw().unit_pair) return false;
    auto plain1x1 = [](const ConvArgs& a) { return a.KH == 1 && a.KW == 1 && a.stride == 1 && a.pad == 0 && a.up == 1 && !a.rowrun && a.splitk == 1; };
    if (!plain1x1(c3) || !plain1x1(c1)) return false;
    if (c1.N != c3.N || c1.H != c3.Ho || c1.W != c3.Wo || c1.M != c3.M || c1.Cin != c3.Cout || c1.x_ld != c1.Cin) return false;
    if (c3.Cout % 128 != 0 || c3.K % 64 != 0 || c3.K > 256 || (c1.Cout != 64 && c1.Cout != 128)) return false;
    if (c3.res_stride != 1 || c3.res_H != c3.Ho || c3.res_W != c3.Wo || c3.res_ld % 4 != 0 || c3.x_ld % 4 != 0) return false;
    if (c3.out_floor != nullptr || c1.out_floor != nullptr || c1.bias != nullptr || c1.residual != nullptr) return false;
    if (c3.out_scale != nullptr || c3.in_scale != nullptr || c1.in_scale == nullptr) return false;
    // the two launches' own routes: the fused kernel repeats the arithmetic of exactly these kernels
    const ConvRoute r3 = conv_route(c3, 4, img3), r1 = conv_route(c1, 4, img1);
    if (!(r1.family == CONV_PACKED && r1.pro == 1 && r1.kg == 1 && r1.reduce == 0)) return false;
    if (r3.family == CONV_IGEMM && r3.operand == 0 && r3.bk == 32 && c3.K == 64 && r3.reduce == 0) f.f32a = 1;
    else if ((r3.family == CONV_ASTAT || (r3.family == CONV_PACKED && r3.pro == 0 && r3.kg == 1)) && r3.reduce == 0) f.f32a = 0;
    else return false;
    f.bm = c1.Cout == 64 ? 64 : 32;
    f.lds_bytes = sn_pair_lds_bytes(f.f32a, f.bm, c3.K);
    f.prof_kind = PK_KERNEL_CONV_UNIT_PAIR + 2 * f.f32a + (f.bm == 64 ? 1 : 0);
    return f.lds_bytes <= SN_PAIR_LDS_MAX;
}

ConvGrid conv_unit_pair_grid(const ConvUnitPairForm& f, const ConvArgs& c3) {
    ConvGrid g{};
    g.gx = cdiv(c3.M, f.bm); g.gy = g.gz = 1;
    g.tiles = g.wgs = g.gx;
    return g;
}

template <int F32A, int BM>
static int launch_unit_pair_one(const ConvUnitPairArgs& P, size_t lds, int gx, hipStream_t st) {
    auto kern = conv_unit_pair_f32_kernel<F32A, BM>;
    static size_t configured = 0;                            // (set up on the first launch, whatever it needs)
    if (const int rc = lds_opt_in(reinterpret_cast<const void*>(kern), lds, SN_PAIR_LDS_MAX, configured, "conv unit pair")) return rc;
    kern<<<gx, 256, lds, st>>>(P);
    SN_LAUNCH_CHECK("conv_unit_pair_f32_kernel");
    return STABNET_OK;
}

int conv_unit_pair_launch(const ConvArgs& c3, const ConvArgs& c1, const float* w3_img, const float* w1_img, hipStream_t st, Prof* prof) {
    ConvUnitPairForm f;
    SN_REQUIRE(conv_unit_pair_form(c3, c1, w3_img != nullptr, w1_img != nullptr, f), "conv unit pair: unsupported pair of convolutions");
    SN_REQUIRE(c3.div_hw_mul != 0 && c1.div_hw_mul != 0, "conv unit pair: conv_plan() not called on both convolutions");
    SN_REQUIRE(c3.x && c3.w && c3.y && c1.y && c1.in_scale && c1.in_shift && w1_img && (f.f32a || w3_img), "conv unit pair: null pointer");
    SN_REQUIRE(c1.x == nullptr || c1.x == c3.y, "conv unit pair: conv1 must read conv3's output");
    ConvUnitPairArgs P;
    P.a = c3;
    P.b = c1;
    if (!f.f32a) P.a.w = w3_img;
    P.b.w = w1_img;
    P.b.x = c3.y;
    const ConvGrid g = conv_unit_pair_grid(f, c3);
    g_last_launch_kind = f.prof_kind;
    const bool rec = prof != nullptr && prof->begin(st);
    int rc;
    if (f.f32a) rc = f.bm == 64 ? launch_unit_pair_one<1, 64>(P, f.lds_bytes, g.gx, st) : launch_unit_pair_one<1, 32>(P, f.lds_bytes, g.gx, st);
    else rc = f.bm == 64 ? launch_unit_pair_one<0, 64>(P, f.lds_bytes, g.gx, st) : launch_unit_pair_one<0, 32>(P, f.lds_bytes, g.gx, st);
    if (rec) prof->end(st, f.prof_kind, 2.0 * c3.M * ((double)c3.K * c3.Cout + (double)c1.K * c1.Cout),
                       // algorithmic bytes: conv3's input + both weights + conv3's output + the residual read + conv1's output
                       4.0 * ((double)c3.M * c3.K + (double)c3.K * c3.Cout + (double)c1.K * c1.Cout + (double)c3.M * c3.Cout * (c3.residual ? 2 : 1) +
                              (double)c1.M * c1.Cout),
                       c3.M, c1.Cout, c3.K + c1.K, 1);
    return rc;
}

// ---------------------------------------------------------------------------------------------------------
const char* conv_extent_over(const ConvArgs& a, long in_floats, bool has_residual, long* floats) {
    const long pixels = (long)a.N * a.H * a.W;
    const long in = in_floats > 0 ? in_floats : pixels * (a.x_ld ? a.x_ld : a.Cin);
    const long out = (long)a.N * a.Ho * a.Wo * a.Cout;
    const long res = has_residual ? (long)a.N * a.res_H * a.res_W * (a.res_ld ? a.res_ld : a.Cout) : 0;
    const long w = (long)a.Cout * (a.K ? a.K : a.KH * a.KW * a.Cin);
    const struct { const char* name; long n; } ops[4] = {{"input", in}, {"output", out}, {"residual", res}, {"weights", w}};
    for (const auto& o : ops)
        if (o.n >= SN_CONV_EXTENT_LIMIT) {
            if (floats) *floats = o.n;
            return o.name;
        }
    return nullptr;
}
// The operator entries' form of it: the input counted over the zero-padded frame, as fill_args() has always counted it (with Cin),
// now with every x_ld column.  Call with x_ld / res_ld set and conv_plan() done.
static int check_extents(const ConvArgs& a, const char* who) {
    long n = 0;
    const long in = (long)a.N * (a.H + 2 * a.pad) * (a.W + 2 * a.pad) * (a.x_ld ? a.x_ld : a.Cin);
    const char* op = conv_extent_over(a, in, a.residual != nullptr, &n);
    SN_REQUIRE(op == nullptr, "%s: the %s spans %ld floats (x_ld=%d, res_ld=%d): every conv operand must stay below 2^30 floats, all x_ld / res_ld columns counted",
               who, op, n, a.x_ld, a.res_ld);
    return STABNET_OK;
}

static int fill_args(ConvArgs& a, const float* x, const float* w, const float* bias, const float* in_scale,
                     const float* in_shift, const float* residual, int res_H, int res_W, int res_stride, float* y,
                     int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int relu_out) {
    SN_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && KH > 0 && KW > 0 && stride > 0 && pad >= 0,
               "conv2d: bad geometry");
    SN_REQUIRE(Cin % 16 == 0, "conv2d: Cin=%d must be a multiple of 16", Cin);
    SN_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "conv2d: in_scale and in_shift go together");
    a = ConvArgs{};
    a.x = x; a.w = w; a.y = y; a.bias = bias; a.in_scale = in_scale; a.in_shift = in_shift; a.residual = residual;
    a.in_scale_expected = in_scale != nullptr ? 1 : 0;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad;
    a.up = 1;
    a.Ho = (H + 2 * pad - KH) / stride + 1;
    a.Wo = (W + 2 * pad - KW) / stride + 1;
    SN_REQUIRE(a.Ho > 0 && a.Wo > 0, "conv2d: empty output");
    a.res_H = residual ? res_H : a.Ho;
    a.res_W = residual ? res_W : a.Wo;
    a.res_stride = residual ? res_stride : 1;
    a.relu_out = relu_out;
    SN_REQUIRE((long)N * a.Ho * a.Wo * Cout < (1L << 30) && (long)N * (H + 2 * pad) * (W + 2 * pad) * Cin < (1L << 30) &&
                   (long)Cout * KH * KW * Cin < (1L << 30), "conv2d: tensors must have < 2^30 elements");
    // the residual's frame as the caller states it, with or without a pointer: a strided one ([N][res_H][res_W][Cout], read at
    // (oy*res_stride, ox*res_stride)) is larger than the output
    const long res_floats = (long)N * (res_H > 0 ? res_H : a.Ho) * (res_W > 0 ? res_W : a.Wo) * Cout;
    SN_REQUIRE(res_floats < SN_CONV_EXTENT_LIMIT, "conv2d: the residual spans %ld floats (res_H=%d, res_W=%d): every conv operand must stay below 2^30 floats",
               res_floats, res_H, res_W);
    SN_REQUIRE(KH * KW <= 64, "conv2d: filter larger than 64 taps");
    return STABNET_OK;
}

extern "C" {

/* CUs the persistent grids (ring, back-to-back, the N groups of the A-stationary and patch kernels) leave free from the next launch
 * on: usable_cus() = max(CUs / 8, CUs - reserved).  A negative value stores 0; returns the previous value.  Which workgroup computes
 * which tile changes with it, the arithmetic of a tile does not: results are bit-identical for every value.  Not thread-safe. */
int stabnet_conv_reserve_cus(int reserved) {
    const int prev = g_reserved_cus;
    g_reserved_cus = reserved < 0 ? 0 : reserved;
    return prev;
}

/* Tuning hook: force the tile (0 = 128x128, 1 = 128x64, 2 = 64x64) and split-K of every subsequent convolution;
 * tile < 0 restores the built-in choice.  Not thread-safe; used by tools/autotune.py and the tests. */
void stabnet_conv_tuning_override(int tile, int splitk) {
    g_force_tile = tile < 0 ? -1 : tile;
    g_force_split = splitk;
}

/* Tuning hook (tools/tune_splitk.py): split-K of the convolution with GEMM shape (M, Cout, K), filter height KH, on the
 * ring kernel (ring = 1: no input BN prologue) or the register-staged kernel (ring = 0); splitk <= 0 removes the entry,
 * M < 0 clears the table.  Takes effect for plans made afterwards (net_create / conv2d calls).  Not thread-safe. */
void stabnet_conv_tuning_profile(int profile) { g_tuning_profile = profile == 1 ? 1 : 0; }

void stabnet_conv_tuning_table_set(int M, int Cout, int K, int KH, int ring, int splitk) {
    if (M < 0) { g_tuning_runtime.clear(); return; }
    for (size_t i = 0; i < g_tuning_runtime.size(); ++i) {
        TuneEntry& e = g_tuning_runtime[i];
        if (e.M == M && e.Cout == Cout && e.K == K && e.KH == KH && e.ring == ring) {
            if (splitk > 0) e.splitk = splitk;
            else g_tuning_runtime.erase(g_tuning_runtime.begin() + i);
            return;
        }
    }
    if (splitk > 0) g_tuning_runtime.push_back({M, Cout, K, KH, ring, splitk});
}

size_t stabnet_conv2d_workspace_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    ConvArgs a;
    if (fill_args(a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 1, nullptr, N, H, W, Cin, Cout, KH, KW,
                  stride, pad, 0))
        return 0;
    // the split-K choice (measured table) depends on whether the launch carries an input prologue, which this query does not
    // know: the larger of the two
    ConvArgs b = a;
    b.in_scale_expected = 1;
    return std::max(conv_plan(a), conv_plan(b));
}

int stabnet_conv2d_fwd_ex(const float* x, const float* w_ohwi, const float* bias, const float* in_scale,
                          const float* in_shift, const float* residual, int res_H, int res_W, int res_stride,
                          const float* out_scale, const float* out_shift, float* y, int N, int H, int W, int Cin,
                          int Cout, int KH, int KW, int stride, int pad, int relu_out, void* workspace,
                          size_t workspace_bytes, void* stream);

int stabnet_conv2d_fwd(const float* x, const float* w_ohwi, const float* bias, const float* in_scale,
                       const float* in_shift, const float* residual, int res_H, int res_W, int res_stride, float* y,
                       int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int relu_out,
                       void* workspace, size_t workspace_bytes, void* stream) {
    return stabnet_conv2d_fwd_ex(x, w_ohwi, bias, in_scale, in_shift, residual, res_H, res_W, res_stride, nullptr, nullptr,
                                 y, N, H, W, Cin, Cout, KH, KW, stride, pad, relu_out, workspace, workspace_bytes, stream);
}

/* The Profiler kind (stabnet_prof_kind_name) of the convolution kernel this thread launched last through conv_launch() -- the forward
 * operators, dgrad, the layers of a plan --, conv_launch_pair() or conv_b2b_launch(): the route the launch itself took with its
 * pointers.  -1 before the first launch.  Host only. */
int stabnet_conv_last_launch_kind(void) { return g_last_launch_kind; }

int stabnet_conv2d_fwd_ex(const float* x, const float* w_ohwi, const float* bias, const float* in_scale,
                          const float* in_shift, const float* residual, int res_H, int res_W, int res_stride,
                          const float* out_scale, const float* out_shift, float* y, int N, int H, int W, int Cin,
                          int Cout, int KH, int KW, int stride, int pad, int relu_out, void* workspace,
                          size_t workspace_bytes, void* stream) {
    SN_REQUIRE(x && w_ohwi && y, "conv2d_fwd: null pointer");
    SN_REQUIRE((out_scale == nullptr) == (out_shift == nullptr), "conv2d_fwd: out_scale and out_shift go together");
    ConvArgs a;
    int rc = fill_args(a, x, w_ohwi, bias, in_scale, in_shift, residual, res_H, res_W, res_stride, y, N, H, W, Cin, Cout,
                       KH, KW, stride, pad, relu_out);
    if (rc) return rc;
    const size_t need = conv_plan(a);
    if (need > workspace_bytes || (need > 0 && workspace == nullptr)) {
        stabnet_set_error("conv2d_fwd: workspace %zu B < %zu B needed", workspace_bytes, need);
        return STABNET_ERR_WORKSPACE;
    }
    a.partial = static_cast<float*>(workspace);
    a.out_scale = out_scale;
    a.out_shift = out_shift;
    return conv_launch(a, (hipStream_t)stream);
}

/* stabnet_conv2d_fwd_ex through the packed split kernels (include/stabnet_hip.h) */
int stabnet_conv2d_fwd_packed_ld(const float* x, int x_ld, const float* w_ohwi, const float* w_img, const float* bias, const float* in_scale,
                                 const float* in_shift, const float* residual, int res_H, int res_W, int res_stride,
                                 const float* out_scale, const float* out_shift, float* y, int N, int H, int W, int Cin,
                                 int Cout, int KH, int KW, int stride, int pad, int relu_out, int splitk, void* workspace,
                                 size_t workspace_bytes, void* stream);
size_t stabnet_conv_weight_image_floats(int Cout, int KH, int KW, int Cin) {
    const int K = KH * KW * Cin;
    return (Cout > 0 && K > 0 && K % 32 == 0) ? conv_weight_image_floats(Cout, K) : 0;
}

int stabnet_conv_weight_split_image(const float* w_ohwi, int Cout, int KH, int KW, int Cin, float* w_img, void* stream) {
    SN_REQUIRE(w_ohwi && w_img, "conv_weight_split_image: null pointer");
    SN_REQUIRE(Cin % 32 == 0, "conv_weight_split_image: Cin=%d must be a multiple of 32", Cin);
    return launch_weight_split_image(w_ohwi, Cout, KH * KW * Cin, w_img, (hipStream_t)stream);
}

/* conv_plan() with the caller's K split (splitk > 0) instead of the planned one; returns the workspace bytes */
static size_t plan_packed(ConvArgs& a, int splitk) {
    size_t need = conv_plan(a);
    if (splitk > 0) {
        const int total = conv_total_steps(a);
        a.steps_per_split = cdiv(total, std::min(splitk, total));
        a.splitk = cdiv(total, a.steps_per_split);
        need = a.splitk > 1 ? (size_t)a.splitk * a.M * a.Cout * sizeof(float) : 0;
    }
    return need;
}

/* The Profiler kind (stabnet_prof_kind_name) of the conv launch stabnet_conv2d_fwd_packed makes for this geometry, with (prologue != 0)
 * or without an input BN + ReLU: conv_route() of the launch bound to placeholders -- prologue vectors, split-K workspace and weight
 * image; every other pointer null.  Host only; < 0 on a bad geometry. */
int stabnet_conv2d_packed_kind(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int prologue, int splitk) {
    ConvArgs a;
    if (fill_args(a, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 1, nullptr, N, H, W, Cin, Cout, KH, KW, stride, pad, 0))
        return STABNET_ERR_BAD_ARG;
    a.in_scale_expected = prologue ? 1 : 0;
    (void)plan_packed(a, splitk);
    if (prologue) { a.in_scale = sn_placeholder_base(1); a.in_shift = a.in_scale + a.Cin; }
    a.partial = sn_placeholder_base(2);
    return conv_route(a, 4, true).prof_kind;              // (the call always comes with an image pointer)
}

int stabnet_conv2d_fwd_packed(const float* x, const float* w_ohwi, const float* w_img, const float* bias, const float* in_scale,
                              const float* in_shift, const float* residual, int res_H, int res_W, int res_stride,
                              const float* out_scale, const float* out_shift, float* y, int N, int H, int W, int Cin,
                              int Cout, int KH, int KW, int stride, int pad, int relu_out, int splitk, void* workspace,
                              size_t workspace_bytes, void* stream) {
    return stabnet_conv2d_fwd_packed_ld(x, 0, w_ohwi, w_img, bias, in_scale, in_shift, residual, res_H, res_W, res_stride, out_scale, out_shift,
                                        y, N, H, W, Cin, Cout, KH, KW, stride, pad, relu_out, splitk, workspace, workspace_bytes, stream);
}

/* stabnet_conv2d_fwd_packed on an input whose pixels lie x_ld floats apart (0 = Cin): Cin columns of a wider buffer */
int stabnet_conv2d_fwd_packed_ld(const float* x, int x_ld, const float* w_ohwi, const float* w_img, const float* bias, const float* in_scale,
                                 const float* in_shift, const float* residual, int res_H, int res_W, int res_stride,
                                 const float* out_scale, const float* out_shift, float* y, int N, int H, int W, int Cin,
                                 int Cout, int KH, int KW, int stride, int pad, int relu_out, int splitk, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    // (the shape is judged before the pointers: a geometry outside the kernels' range is refused whatever it comes with)
    SN_REQUIRE(x_ld == 0 || (x_ld >= Cin && x_ld % 4 == 0), "conv2d_fwd_packed: x_ld=%d must be 0 or a multiple of 4 >= Cin=%d", x_ld, Cin);
    ConvArgs a;
    int rc = fill_args(a, x, w_ohwi, bias, in_scale, in_shift, residual, res_H, res_W, res_stride, y, N, H, W, Cin, Cout,
                       KH, KW, stride, pad, relu_out);
    if (rc) return rc;
    a.x_ld = x_ld;
    const size_t need = plan_packed(a, splitk);
    if ((rc = check_extents(a, "conv2d_fwd_packed")) != 0) return rc;
    SN_REQUIRE(x && w_ohwi && w_img && y, "conv2d_fwd_packed: null pointer");
    SN_REQUIRE((out_scale == nullptr) == (out_shift == nullptr), "conv2d_fwd_packed: out_scale and out_shift go together");
    if (need > workspace_bytes || (need > 0 && workspace == nullptr)) {
        stabnet_set_error("conv2d_fwd_packed: workspace %zu B < %zu B needed", workspace_bytes, need);
        return STABNET_ERR_WORKSPACE;
    }
    a.partial = static_cast<float*>(workspace);
    a.out_scale = out_scale;
    a.out_shift = out_shift;
    return conv_launch(a, (hipStream_t)stream, nullptr, 4, w_img);
}

/* conv3 -> next unit's conv1 as one launch (include/stabnet_hip.h) */
int stabnet_conv_unit_pair_fwd(const float* x, const float* w3_ohwi, const float* w3_img, const float* bias3, const float* residual, int res_ld,
                               const float* pre_scale, const float* pre_shift, const float* w1_ohwi, const float* w1_img, const float* out_scale,
                               const float* out_shift, float* y3, float* y1, int N, int H, int W, int K1, int N1, int N2, int relu_out, void* stream) {
    // (the shapes are judged before the pointers; res_ld counts whether or not this call reads a residual)
    SN_REQUIRE(res_ld == 0 || (res_ld >= N1 && res_ld % 4 == 0), "conv_unit_pair_fwd: res_ld=%d must be 0 or a multiple of 4 >= N1=%d", res_ld, N1);
    ConvArgs c3, c1;
    int rc = fill_args(c3, x, w3_ohwi, bias3, nullptr, nullptr, residual, H, W, 1, y3, N, H, W, K1, N1, 1, 1, 1, 0, 0);
    if (rc) return rc;
    c3.res_ld = res_ld;
    (void)plan_packed(c3, 1);
    rc = fill_args(c1, y3, w1_ohwi, nullptr, pre_scale, pre_shift, nullptr, 0, 0, 1, y1, N, H, W, N1, N2, 1, 1, 1, 0, relu_out);
    if (rc) return rc;
    (void)plan_packed(c1, 1);
    long ext = 0;
    const char* over = conv_extent_over(c3, 0, true, &ext);
    SN_REQUIRE(over == nullptr, "conv_unit_pair_fwd: conv3's %s spans %ld floats (res_ld=%d): every conv operand must stay below 2^30 floats, all res_ld columns counted",
               over, ext, c3.res_ld);
    if ((rc = check_extents(c1, "conv_unit_pair_fwd (conv1)")) != 0) return rc;
    SN_REQUIRE(x && w3_ohwi && pre_scale && pre_shift && w1_ohwi && w1_img && y3 && y1, "conv_unit_pair_fwd: null pointer");
    SN_REQUIRE((out_scale == nullptr) == (out_shift == nullptr), "conv_unit_pair_fwd: out_scale and out_shift go together");
    c1.out_scale = out_scale;
    c1.out_shift = out_shift;
    return conv_unit_pair_launch(c3, c1, w3_img, w1_img, (hipStream_t)stream);
}

/* conv2 (3x3, pad 1, stride 1 | 2, C -> C channels, C = 64 | 128, no bias) -> folded BN (mid_scale, mid_shift) + ReLU -> conv3
 * (1x1, C -> Cout, Cout % C == 0) with conv2d_fwd_ex's epilogue (bias, residual, out_scale / out_shift, relu_out) as ONE launch:
 * the tail of a slim bottleneck_v2 unit (s_net_bundle_nobm.py:252-253); the C-channel intermediate never reaches memory.
 * x [N,H,W,C] with x_ld floats between pixels (0 = C); y [N,Ho,Wo,Cout]; residual read at (oy*res_stride, ox*res_stride) with
 * res_ld floats between pixels (0 = Cout).  STABNET_ERR_BAD_ARG for other geometries. */
int stabnet_conv3x3_conv1x1_fwd(const float* x, int x_ld, const float* w2_ohwi, const float* mid_scale, const float* mid_shift,
                                const float* w3_ohwi, const float* bias3, const float* residual, int res_H, int res_W,
                                int res_stride, int res_ld, const float* out_scale, const float* out_shift, float* y, int N, int H,
                                int W, int C, int Cout, int stride, int relu_out, void* stream) {
    // (the shapes are judged before the pointers; res_ld counts whether or not this call reads a residual)
    SN_REQUIRE(x_ld == 0 || (x_ld >= C && x_ld % 4 == 0), "conv3x3_conv1x1_fwd: x_ld=%d must be 0 or a multiple of 4 >= C=%d", x_ld, C);
    SN_REQUIRE(res_ld == 0 || (res_ld >= Cout && res_ld % 4 == 0), "conv3x3_conv1x1_fwd: res_ld=%d must be 0 or a multiple of 4 >= Cout=%d", res_ld, Cout);
    ConvArgs c2, c3;
    int rc = fill_args(c2, x, w2_ohwi, nullptr, nullptr, nullptr, nullptr, 0, 0, 1, nullptr, N, H, W, C, C, 3, 3, stride, 1, 1);
    if (rc) return rc;
    c2.x_ld = x_ld;
    (void)conv_plan(c2);
    if ((rc = check_extents(c2, "conv3x3_conv1x1_fwd (conv2)")) != 0) return rc;
    c2.out_scale = mid_scale;
    c2.out_shift = mid_shift;
    rc = fill_args(c3, nullptr, w3_ohwi, bias3, nullptr, nullptr, residual, res_H, res_W, res_stride, y, N, c2.Ho, c2.Wo, C, Cout,
                   1, 1, 1, 0, relu_out);
    if (rc) return rc;
    c3.res_ld = res_ld;
    (void)conv_plan(c3);
    {
        long ext = 0;
        ConvArgs t = c3;                                   // (the residual's frame as the caller states it, with or without a pointer)
        if (res_H > 0 && res_W > 0) { t.res_H = res_H; t.res_W = res_W; }
        const char* over = conv_extent_over(t, 0, true, &ext);
        SN_REQUIRE(over == nullptr, "conv3x3_conv1x1_fwd: conv3's %s spans %ld floats (res_ld=%d): every conv operand must stay below 2^30 floats, all res_ld columns counted",
                   over, ext, c3.res_ld);
    }
    SN_REQUIRE(x && w2_ohwi && mid_scale && mid_shift && w3_ohwi && y, "conv3x3_conv1x1_fwd: null pointer");
    SN_REQUIRE((out_scale == nullptr) == (out_shift == nullptr), "conv3x3_conv1x1_fwd: out_scale and out_shift go together");
    c3.out_scale = out_scale;
    c3.out_shift = out_shift;
    SN_REQUIRE(conv_b2b_supported(c2, c3), "conv3x3_conv1x1_fwd: C must be 64 or 128, Cout a multiple of C, stride 1 or 2");
    return conv_b2b_launch(c2, c3, (hipStream_t)stream);
}

}  // extern "C"
