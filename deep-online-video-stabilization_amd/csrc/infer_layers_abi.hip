// C entry points of the inference layers and head (layers.hip, head.hip), one per operator (include/stabnet_hip.h): the deployed
// frame reaches these kernels through the plan of net.hip, which hands their launchers shapes it has laid out itself; the operator
// tests reach the SAME launchers through these, so every shape, alignment and pointer is checked here, before the first launch.
#include "layers.h"
#include <initializer_list>

static int check_device_all(std::initializer_list<const void*> ptrs, const char* what, hipStream_t st) {
    for (const void* p : ptrs)
        if (p != nullptr)
            if (int rc = sn_check_device(p, what, st)) return rc;
    return STABNET_OK;
}

static bool aligned16(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (((size_t)p & 15) != 0) return false;
    return true;
}

extern "C" {

int stabnet_pad_channels(const float* x, float* y, long npix, int C, int Cp, void* stream) {
    SN_REQUIRE(x && y, "pad_channels: null pointer");
    SN_REQUIRE(npix > 0 && C > 0 && Cp >= C && Cp % 4 == 0 && npix * (Cp / 4) < (1L << 31) * 256,
               "pad_channels: npix = %ld, channels %d -> %d (the padded count is a multiple of 4, not below C)", npix, C, Cp);
    SN_REQUIRE(aligned16({y}), "pad_channels: y is not 16-byte aligned");
    if (int rc = check_device_all({x, y}, "pad_channels: an argument", (hipStream_t)stream)) return rc;
    return launch_pad_channels(x, y, npix, C, Cp, (hipStream_t)stream);
}

int stabnet_stem_repack(const float* w, float* out, int Cout, int KH, int KW, int CinPad, int Cin, void* stream) {
    SN_REQUIRE(w && out, "stem_repack: null pointer");
    SN_REQUIRE(Cout > 0 && KH > 0 && KW > 0 && Cin > 0 && CinPad >= Cin && (long)KW * Cin < (1L << 20) &&
               (long)Cout * KH * (((long)KW * Cin + 31) / 32 * 32) < (1L << 31),
               "stem_repack: Cout = %d, %d x %d taps, Cin = %d in rows of %d (CinPad >= Cin, fewer than 2^31 outputs)", Cout, KH, KW, Cin, CinPad);
    if (int rc = check_device_all({w, out}, "stem_repack: an argument", (hipStream_t)stream)) return rc;
    return launch_stem_repack(w, out, Cout, KH, KW, CinPad, Cin, (hipStream_t)stream);
}

int stabnet_merge_vectors(const float* b_sc, const float* scale1, const float* shift1, int depth, int dbn, float* out, void* stream) {
    SN_REQUIRE(b_sc && scale1 && shift1 && out, "merge_vectors: null pointer");
    SN_REQUIRE(depth > 0 && dbn > 0 && (long)depth + dbn < (1L << 28), "merge_vectors: depth = %d, dbn = %d", depth, dbn);
    if (int rc = check_device_all({b_sc, scale1, shift1, out}, "merge_vectors: an argument", (hipStream_t)stream)) return rc;
    return launch_merge_vectors(b_sc, scale1, shift1, depth, dbn, out, (hipStream_t)stream);
}

int stabnet_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int G, float* scale,
                    float* shift, void* stream) {
    SN_REQUIRE(gamma && beta && mean && var && scale && shift, "bn_fold: null pointer");
    SN_REQUIRE(G > 0, "bn_fold: G = %d", G);
    if (int rc = check_device_all({gamma, beta, mean, var, scale, shift}, "bn_fold: an argument", (hipStream_t)stream)) return rc;
    return launch_bn_fold(gamma, beta, mean, var, eps, G, scale, shift, (hipStream_t)stream);
}

int stabnet_max_pool_fwd(const float* x, float* y, int N, int H, int W, int C, int Ho, int Wo, int k, int stride, int pt, int pl,
                         const float* scale, const float* shift, void* stream) {
    SN_REQUIRE(x && y, "max_pool_fwd: null pointer");
    SN_REQUIRE((scale == nullptr) == (shift == nullptr), "max_pool_fwd: scale and shift come together (both or neither)");
    SN_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && Ho > 0 && Wo > 0 && k > 0 && stride > 0 && pt >= 0 && pl >= 0 && pt < k && pl < k &&
               (long)(Ho - 1) * stride - pt < H && (long)(Wo - 1) * stride - pl < W, "max_pool_fwd: bad geometry (a window outside the image)");
    SN_REQUIRE(C % 4 == 0, "max_pool_fwd: C = %d (C %% 4 != 0)", C);
    SN_REQUIRE((double)N * Ho * Wo * (C / 4) < 4294967296.0, "max_pool_fwd: more than 2^32 channel quads (%d x %d x %d x %d / 4)", N, Ho, Wo, C);
    SN_REQUIRE(aligned16({x, y, scale, shift}), "max_pool_fwd: a pointer is not 16-byte aligned");
    if (int rc = check_device_all({x, y, scale, shift}, "max_pool_fwd: an argument", (hipStream_t)stream)) return rc;
    return launch_max_pool(x, y, N, H, W, C, Ho, Wo, k, stride, pt, pl, scale, shift, (hipStream_t)stream);
}

static bool gap_shape_ok(int N, int HW, int C) { return N > 0 && N <= 65535 && HW > 0 && C > 0 && (long)HW * C < (1L << 40); }

size_t stabnet_gap_partial_floats(int N, int HW, int C) {
    if (!gap_shape_ok(N, HW, C) || C % 4 != 0) return 0;
    return (size_t)N * gap_chunks(HW) * C;
}

int stabnet_gap_bn_relu(const float* x, const float* scale, const float* shift, int N, int HW, int C, float* out, float* partial,
                        size_t partial_floats, void* stream) {
    SN_REQUIRE(x && scale && shift && out && partial, "gap_bn_relu: null pointer");
    SN_REQUIRE(gap_shape_ok(N, HW, C), "gap_bn_relu: N = %d (1..65535), HW = %d, C = %d", N, HW, C);
    SN_REQUIRE(C % 4 == 0, "gap_bn_relu: C = %d (C %% 4 != 0)", C);
    SN_REQUIRE(partial_floats >= stabnet_gap_partial_floats(N, HW, C), "gap_bn_relu: partial holds %zu floats, %zu are needed",
               partial_floats, stabnet_gap_partial_floats(N, HW, C));
    SN_REQUIRE(aligned16({x, scale, shift, partial}), "gap_bn_relu: a pointer is not 16-byte aligned");
    if (int rc = check_device_all({x, scale, shift, out, partial}, "gap_bn_relu: an argument", (hipStream_t)stream)) return rc;
    return launch_gap_bn_relu(x, scale, shift, N, HW, C, out, partial, (hipStream_t)stream);
}

int stabnet_fc_fwd(const float* x, const float* w, const float* b, float* y, int M, int K, int Nout, int relu, void* stream) {
    SN_REQUIRE(x && w && y, "fc_fwd: null pointer");
    SN_REQUIRE(M > 0 && K > 0 && Nout > 0 && (long)M * K < (1L << 31) && (long)Nout * K < (1L << 40), "fc_fwd: M = %d, K = %d, Nout = %d", M, K, Nout);
    SN_REQUIRE(K % 4 == 0, "fc_fwd: K = %d (K %% 4 != 0)", K);
    SN_REQUIRE(aligned16({x, w}), "fc_fwd: x or w is not 16-byte aligned");
    if (int rc = check_device_all({x, w, b, y}, "fc_fwd: an argument", (hipStream_t)stream)) return rc;
    return launch_fc(x, w, b, y, M, K, Nout, relu ? 1 : 0, (hipStream_t)stream);
}

int stabnet_head_fused_supported(int N, int C, const int* fc_dims) {
    if (fc_dims == nullptr) return 0;
    return head_fused_supported(N, C, fc_dims);
}

static bool head_gap_shape_ok(int N, int HW, int C) { return N >= 1 && N <= 8 && HW > 0 && C > 0 && C <= 2048 && C % 64 == 0; }

size_t stabnet_head_gap_partial_floats(int N, int HW, int C) {
    if (!head_gap_shape_ok(N, HW, C)) return 0;
    return (size_t)N * head_gap_chunks(N, HW) * C;
}

int stabnet_head_gap_fc1(const float* x, const float* scale, const float* shift, int N, int HW, int C, float* partial,
                         size_t partial_floats, float* gap_out, const float* w, const float* b, float* y, int Nout, void* stream) {
    SN_REQUIRE(x && scale && shift && partial && w && b && y, "head_gap_fc1: null pointer");
    SN_REQUIRE(N >= 1 && N <= 8, "head_gap_fc1: N = %d (1..8: fc_1's activations are staged in 64 KiB of LDS)", N);
    SN_REQUIRE(C > 0 && C <= 2048 && C % 64 == 0, "head_gap_fc1: C = %d (C %% 64 != 0 or C > 2048)", C);
    SN_REQUIRE(HW > 0 && Nout > 0 && (long)Nout * C < (1L << 40), "head_gap_fc1: HW = %d, Nout = %d", HW, Nout);
    SN_REQUIRE(partial_floats >= stabnet_head_gap_partial_floats(N, HW, C), "head_gap_fc1: partial holds %zu floats, %zu are needed",
               partial_floats, stabnet_head_gap_partial_floats(N, HW, C));
    SN_REQUIRE(aligned16({x, scale, shift, partial, gap_out, w}), "head_gap_fc1: a pointer is not 16-byte aligned");
    if (int rc = check_device_all({x, scale, shift, partial, gap_out, w, b, y}, "head_gap_fc1: an argument", (hipStream_t)stream)) return rc;
    return launch_gap_fc1(x, scale, shift, N, HW, C, partial, gap_out, w, b, y, Nout, (hipStream_t)stream);
}

int stabnet_head_theta_mesh(const float* x, const float* w, const float* b, int N, int K, int n_theta, float* theta, int grid_h,
                            int grid_w, float do_crop_rate, float* Hs, int* head_adv, int depth, const float* prefetch_src, int pf_H,
                            int pf_W, void* stream) {
    SN_REQUIRE(x && w && b && theta, "head_theta_mesh: null pointer");
    SN_REQUIRE(K == 512, "head_theta_mesh: K = %d (the kernel is built for the 512 outputs of fc_3)", K);
    SN_REQUIRE(N > 0 && N <= (1 << 20), "head_theta_mesh: N = %d", N);
    SN_REQUIRE(n_theta >= 1 && n_theta <= 64, "head_theta_mesh: n_theta = %d (1..64: 16 rows on each of the 4 waves)", n_theta);
    SN_REQUIRE(grid_h >= 1 && grid_w >= 1 && (long)grid_h * grid_w <= 64, "head_theta_mesh: gh*gw = %d x %d (1..64 cells)", grid_h, grid_w);
    if (Hs != nullptr) {
        SN_REQUIRE(n_theta == 2 * (grid_h + 1) * (grid_w + 1), "head_theta_mesh: Hs of a %d x %d mesh needs n_theta = %d, not %d", grid_h,
                   grid_w, 2 * (grid_h + 1) * (grid_w + 1), n_theta);
        SN_REQUIRE(do_crop_rate > 0.f, "head_theta_mesh: do_crop_rate must be > 0");
    }
    SN_REQUIRE(head_adv == nullptr || depth >= 1, "head_theta_mesh: depth = %d of the ring whose head is advanced", depth);
    SN_REQUIRE(prefetch_src == nullptr || (pf_H > 0 && pf_W > 0), "head_theta_mesh: prefetch frame of %d x %d", pf_H, pf_W);
    SN_REQUIRE(aligned16({x, w}) && ((size_t)head_adv & 3) == 0, "head_theta_mesh: x or w is not 16-byte aligned (or head_adv not 4-byte)");
    if (int rc = check_device_all({x, w, b, theta, Hs, head_adv, prefetch_src}, "head_theta_mesh: an argument", (hipStream_t)stream)) return rc;
    return launch_theta_mesh(x, w, b, N, n_theta, theta, grid_h, grid_w, Hs != nullptr ? 1.0f / do_crop_rate : 0.f, Hs, head_adv,
                             head_adv != nullptr ? depth : 1, (hipStream_t)stream, prefetch_src, pf_H, pf_W);
}

}  // extern "C"
