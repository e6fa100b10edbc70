// C entry points onto the launchers a backward stage of the training step runs (run_backward_stage, net.hip): the two-tower wgrad
// with ONE reduce table and slab cursor over several layers, the table forms of the dgrad weight re-pack and of the weight images,
// and dgrad on the packed split kernels.  The step hands these launchers shapes and offsets of its own plan; the operator tests
// reach the SAME launchers through these, so every shape, alignment, capacity and pointer is checked here, before the first launch.
#include "conv.h"
#include "train_layers.h"
#include <vector>

namespace {

struct WgradLayer { int N, H, W, Cin, Cout, KH, KW, stride, pad, M, K; };

// a * b * c * d < 2^31 for factors in [0, 2^31], without overflow: the running product is cut off as soon as it reaches the limit
bool below_2_31(long a, long b, long c = 1, long d = 1) {
    long p = a;
    for (long f : {b, c, d}) {
        if (p >= (1L << 31)) return false;
        p *= f;
    }
    return p < (1L << 31);
}

// geom: N, H, W, Cin, Cout, KH, KW, stride, pad -- the limits are wgrad_launch_g's own (and the int ranges of what it derives)
bool wgrad_layer_ok(const int* g, WgradLayer& o) {
    o = {g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], 0, 0};
    if (o.N <= 0 || o.H <= 0 || o.W <= 0 || o.Cin <= 0 || o.Cout <= 0 || o.KH <= 0 || o.KW <= 0 || o.stride <= 0 || o.pad < 0) return false;
    if (o.H > (1 << 20) || o.W > (1 << 20) || o.pad > 64 || o.KH > 64 || o.KW > 64 || o.Cin > (1 << 20) || o.Cout > (1 << 20)) return false;
    if (o.Cin % 4 != 0 || o.Cout % 4 != 0 || o.KH > o.H + 2 * o.pad || o.KW > o.W + 2 * o.pad) return false;
    const long Ho = (o.H + 2 * o.pad - o.KH) / o.stride + 1, Wo = (o.W + 2 * o.pad - o.KW) / o.stride + 1;
    const long K = (long)o.KH * o.KW * o.Cin;                  // (< 2^32: the factors are bounded above)
    if (!below_2_31(o.N, Ho, Wo, o.Cout) || !below_2_31((long)o.N + 1, o.H + 2 * o.pad, o.W + 2 * o.pad, o.Cin) || !below_2_31(K, o.Cout)) return false;
    o.M = (int)(o.N * Ho * Wo); o.K = (int)K;
    return true;
}

bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

size_t round256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// the dgrad of a forward conv as the convolution dgrad_launch() runs (planned: tile and K split chosen)
bool dgrad_geometry_ok(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad < 0) return false;
    if (H > (1 << 20) || W > (1 << 20) || KH > 64 || KW > 64 || stride > 64 || Cin > (1 << 20) || Cout > (1 << 20)) return false;
    if (pad > KH - 1 || pad > KW - 1 || KH != KW || KH > H + 2 * pad || KW > W + 2 * pad || Cout % 16 != 0 || Cin % 4 != 0) return false;
    const long Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
    return below_2_31(N, H, W, Cin) && below_2_31(N, Ho, Wo, Cout) && below_2_31(Cout, KH * KW, Cin);
}
size_t dgrad_plan_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    ConvArgs a{};
    a.N = N; a.H = (H + 2 * pad - KH) / stride + 1; a.W = (W + 2 * pad - KW) / stride + 1; a.Cin = Cout; a.Cout = Cin; a.KH = KH; a.KW = KW;
    a.stride = 1; a.pad = KH - 1 - pad; a.up = stride; a.Ho = H; a.Wo = W;
    return conv_plan(a);
}
size_t dgrad_image_floats(int Cin, int Cout, int KH, int KW) {       // the step's rule (net.hip, the dgrad image table)
    const int Kd = KH * KW * Cout;
    return Kd % 32 == 0 ? conv_weight_image_floats(Cin, Kd) : 0;
}

}  // namespace

extern "C" {

/* see include/stabnet_hip.h */
size_t stabnet_conv2d_wgrad_layers_workspace_bytes(int L, int T, const int* geom, const long* bias_off) {
    if (L <= 0 || L > 4096 || T < 1 || T > 2 || geom == nullptr) return 0;
    size_t floats = 0;
    for (int i = 0; i < L; ++i) {
        WgradLayer g;
        if (!wgrad_layer_ok(geom + 9 * i, g)) return 0;
        floats += wgrad_slab_floats(g.Cout, g.K, g.M, T, bias_off != nullptr && bias_off[2 * i] >= 0);
    }
    return floats * sizeof(float);
}

int stabnet_conv2d_wgrad_layers(int L, int T, const int* geom, const float* const* tensors, float* grads, size_t grads_floats,
                                const long* dw_off, const long* bias_off, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SN_REQUIRE(geom && tensors && grads && dw_off, "conv2d_wgrad_layers: null pointer");
    SN_REQUIRE(L >= 1 && L <= 4096, "conv2d_wgrad_layers: L = %d (1..4096 layers)", L);
    SN_REQUIRE(T == 1 || T == 2, "conv2d_wgrad_layers: T = %d (1 or 2 towers)", T);
    SN_REQUIRE(aligned16(grads) && aligned16(workspace), "conv2d_wgrad_layers: grads or workspace is not 16-byte aligned");
    std::vector<WgradLayer> ly(L);
    size_t need = 0;
    for (int i = 0; i < L; ++i) {
        WgradLayer& g = ly[i];
        SN_REQUIRE(wgrad_layer_ok(geom + 9 * i, g), "conv2d_wgrad_layers: layer %d: bad geometry (channel counts are multiples of 4, tensors < 2^31 elements)", i);
        const long b1 = bias_off ? bias_off[2 * i] : -1, b2 = bias_off ? bias_off[2 * i + 1] : -1;
        SN_REQUIRE(b1 >= -1 && b2 >= -1 && (b1 >= 0 || b2 < 0), "conv2d_wgrad_layers: layer %d: bias offsets %ld, %ld (-1 = none; no second without a first)", i, b1, b2);
        SN_REQUIRE(b1 < 0 || wgrad_bias_fusable(g.N, g.H, g.W, g.Cin, g.Cout, g.KH, g.KW, g.stride, g.pad),
                   "conv2d_wgrad_layers: layer %d cannot carry its bias gradient (1x1 stride-1 layers with Cout %% 256 == 0 only)", i);
        const size_t elems = (size_t)g.Cout * g.K;
        SN_REQUIRE(dw_off[i] >= 0 && dw_off[i] % 4 == 0 && (size_t)dw_off[i] + elems <= grads_floats,
                   "conv2d_wgrad_layers: layer %d: dw at float %ld (+ %zu) of %zu: out of range or not 16-byte aligned", i, dw_off[i], elems, grads_floats);
        for (long b : {b1, b2})
            SN_REQUIRE(b < 0 || (b % 4 == 0 && (size_t)b + g.Cout <= grads_floats),
                       "conv2d_wgrad_layers: layer %d: d_bias at float %ld (+ %d) of %zu: out of range or not 16-byte aligned", i, b, g.Cout, grads_floats);
        const float* const* p = tensors + (size_t)i * T * 4;
        for (int t = 0; t < T; ++t) {
            const float *x = p[4 * t], *dy = p[4 * t + 1], *sc = p[4 * t + 2], *sh = p[4 * t + 3];
            SN_REQUIRE(x && dy, "conv2d_wgrad_layers: layer %d tower %d: null x or dy", i, t);
            SN_REQUIRE((sc == nullptr) == (sh == nullptr) && (sc == nullptr) == (p[2] == nullptr),
                       "conv2d_wgrad_layers: layer %d tower %d: in_scale and in_shift go together, for both towers or neither", i, t);
            SN_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(sc) && aligned16(sh), "conv2d_wgrad_layers: layer %d tower %d: a tensor is not 16-byte aligned", i, t);
            for (const float* q : {x, dy, sc, sh})
                if (q != nullptr)
                    if (int rc = sn_check_device(q, "conv2d_wgrad_layers: a layer tensor", st)) return rc;
        }
        need += wgrad_slab_floats(g.Cout, g.K, g.M, T, b1 >= 0);
    }
    SN_REQUIRE(workspace_bytes >= need * sizeof(float) && (need == 0 || workspace != nullptr),
               "conv2d_wgrad_layers: workspace of %zu B, %zu B are needed", workspace_bytes, need * sizeof(float));
    if (int rc = sn_check_device(grads, "conv2d_wgrad_layers: grads", st)) return rc;
    if (need > 0)
        if (int rc = sn_check_device(workspace, "conv2d_wgrad_layers: workspace", st)) return rc;

    // what a backward stage does: one table, one cursor, one launch per layer for all towers, the ordered reduction at the end
    WgradReduceTable table{};
    size_t cursor = 0;
    for (int i = 0; i < L; ++i) {
        const WgradLayer& g = ly[i];
        const float* const* p = tensors + (size_t)i * T * 4;
        const float *xs[2] = {}, *dys[2] = {}, *sc[2] = {}, *sh[2] = {};
        for (int t = 0; t < T; ++t) { xs[t] = p[4 * t]; dys[t] = p[4 * t + 1]; sc[t] = p[4 * t + 2]; sh[t] = p[4 * t + 3]; }
        const bool pro = sc[0] != nullptr;
        int rc = wgrad_launch_g(T, xs, dys, grads, dw_off[i], pro ? sc : nullptr, pro ? sh : nullptr, g.N, g.H, g.W, g.Cin, g.Cout, g.KH, g.KW,
                                g.stride, g.pad, static_cast<float*>(workspace), &cursor, need, &table, st, nullptr, 0,
                                bias_off ? bias_off[2 * i] : -1, bias_off ? bias_off[2 * i + 1] : -1);
        if (rc) return rc;
    }
    return wgrad_reduce_flush(grads, table, st);
}

int stabnet_pack_dgrad_weights_table(const float* params, size_t params_floats, float* wt, size_t wt_floats, int L, const long* w_off,
                                     const int* dims, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SN_REQUIRE(params && wt && w_off && dims, "pack_dgrad_weights_table: null pointer");
    SN_REQUIRE(L >= 1 && L <= (int)(sizeof(PackTable::d) / sizeof(PackDesc)), "pack_dgrad_weights_table: L = %d (1..%d entries)", L,
               (int)(sizeof(PackTable::d) / sizeof(PackDesc)));
    PackTable t{};
    for (int i = 0; i < L; ++i) {
        const int Cout = dims[4 * i], K = dims[4 * i + 1], Cin = dims[4 * i + 2], stride = dims[4 * i + 3];
        SN_REQUIRE(Cout > 0 && K > 0 && K <= 64 && Cin > 0 && stride > 0 && below_2_31(Cout, K * K, Cin),
                   "pack_dgrad_weights_table: entry %d: Cout = %d, K = %d, Cin = %d, stride = %d", i, Cout, K, Cin, stride);
        const size_t elems = (size_t)Cout * K * K * Cin;
        SN_REQUIRE(w_off[i] >= 0 && (size_t)w_off[i] + elems <= params_floats, "pack_dgrad_weights_table: entry %d: floats %ld .. + %zu of %zu", i,
                   w_off[i], elems, params_floats);
        t.d[i] = {w_off[i], Cout, K, Cin, dgrad_kperm(K, K, stride)};
        t.prefix[i + 1] = t.prefix[i] + (long)elems;
    }
    t.n = L;
    SN_REQUIRE((size_t)t.prefix[L] <= wt_floats && t.prefix[L] < (1L << 31) * 256, "pack_dgrad_weights_table: wt holds %zu floats, %ld are needed", wt_floats, t.prefix[L]);
    if (int rc = sn_check_device(params, "pack_dgrad_weights_table: params", st)) return rc;
    if (int rc = sn_check_device(wt, "pack_dgrad_weights_table: wt", st)) return rc;
    return pack_dgrad_weights_all(params, wt, t, st);
}

int stabnet_conv_weight_split_images_table(const float* w_base, size_t w_floats, float* img_base, size_t img_floats, int L,
                                           const long* w_off, const long* img_off, const int* dims, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SN_REQUIRE(w_base && img_base && w_off && img_off && dims, "conv_weight_split_images_table: null pointer");
    SN_REQUIRE(L >= 1 && L <= 64, "conv_weight_split_images_table: L = %d (1..64 entries)", L);
    SN_REQUIRE(aligned16(w_base) && aligned16(img_base), "conv_weight_split_images_table: w_base or img_base is not 16-byte aligned");
    WeightImageTable t{};
    for (int i = 0; i < L; ++i) {
        const int Cout = dims[2 * i], K = dims[2 * i + 1];
        SN_REQUIRE(Cout > 0 && K > 0 && K % 32 == 0 && below_2_31(Cout, K), "conv_weight_split_images_table: entry %d: Cout = %d, K = %d (K %% 32 != 0)", i, Cout, K);
        SN_REQUIRE(w_off[i] >= 0 && w_off[i] % 4 == 0 && (size_t)w_off[i] + (size_t)Cout * K <= w_floats,
                   "conv_weight_split_images_table: entry %d: weights at float %ld of %zu: out of range or not 16-byte aligned", i, w_off[i], w_floats);
        SN_REQUIRE(img_off[i] >= 0 && img_off[i] % 4 == 0 && (size_t)img_off[i] + conv_weight_image_floats(Cout, K) <= img_floats,
                   "conv_weight_split_images_table: entry %d: image at float %ld of %zu: out of range or not 16-byte aligned", i, img_off[i], img_floats);
        weight_image_table_add(t, w_off[i], img_off[i], Cout, K);
    }
    SN_REQUIRE(t.tprefix[L] < (1L << 31) * 256, "conv_weight_split_images_table: too many weights for one launch");
    if (int rc = sn_check_device(w_base, "conv_weight_split_images_table: w_base", st)) return rc;
    if (int rc = sn_check_device(img_base, "conv_weight_split_images_table: img_base", st)) return rc;
    return launch_weight_split_images(w_base, img_base, t, st);
}

size_t stabnet_conv2d_dgrad_split_workspace_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    if (!dgrad_geometry_ok(N, H, W, Cin, Cout, KH, KW, stride, pad)) return 0;
    return round256((size_t)Cout * KH * KW * Cin * sizeof(float)) + round256(dgrad_image_floats(Cin, Cout, KH, KW) * sizeof(float)) +
           dgrad_plan_bytes(N, H, W, Cin, Cout, KH, KW, stride, pad);
}

int stabnet_conv2d_dgrad_split(const float* dy, const float* w_ohwi, float* dx, const float* residual, int N, int H, int W, int Cin,
                               int Cout, int KH, int KW, int stride, int pad, void* workspace, size_t workspace_bytes,
                               int* packed_route, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SN_REQUIRE(dy && w_ohwi && dx && workspace, "conv2d_dgrad_split: null pointer");
    SN_REQUIRE(dgrad_geometry_ok(N, H, W, Cin, Cout, KH, KW, stride, pad),
               "conv2d_dgrad_split: bad geometry (square filter, pad < K, Cout %% 16 == 0, Cin %% 4 == 0, tensors < 2^31 elements)");
    SN_REQUIRE(workspace_bytes >= stabnet_conv2d_dgrad_split_workspace_bytes(N, H, W, Cin, Cout, KH, KW, stride, pad),
               "conv2d_dgrad_split: workspace of %zu B, %zu B are needed", workspace_bytes,
               stabnet_conv2d_dgrad_split_workspace_bytes(N, H, W, Cin, Cout, KH, KW, stride, pad));
    SN_REQUIRE(aligned16(dy) && aligned16(w_ohwi) && aligned16(dx) && aligned16(residual) && aligned16(workspace),
               "conv2d_dgrad_split: a pointer is not 16-byte aligned");
    for (const void* q : {(const void*)dy, (const void*)w_ohwi, (const void*)dx, (const void*)residual, (const void*)workspace})
        if (q != nullptr)
            if (int rc = sn_check_device(q, "conv2d_dgrad_split: an argument", st)) return rc;
    const size_t wfloats = (size_t)Cout * KH * KW * Cin, img_floats = dgrad_image_floats(Cin, Cout, KH, KW);
    float* wt = static_cast<float*>(workspace);
    float* img = reinterpret_cast<float*>(static_cast<char*>(workspace) + round256(wfloats * sizeof(float)));
    const size_t off = round256(wfloats * sizeof(float)) + round256(img_floats * sizeof(float));
    // the step's order: the re-pack table, the image table over the re-packed weights [Cin][KH * KW * Cout], the dgrad launch
    PackTable pt{};
    pt.d[0] = {0, Cout, KH, Cin, dgrad_kperm(KH, KW, stride)};
    pt.prefix[1] = (long)wfloats;
    pt.n = 1;
    int rc = pack_dgrad_weights_all(w_ohwi, wt, pt, st);
    if (rc) return rc;
    if (img_floats > 0) {
        WeightImageTable it{};
        weight_image_table_add(it, 0, 0, Cin, KH * KW * Cout);
        if ((rc = launch_weight_split_images(wt, img, it, st)) != 0) return rc;
    }
    int packed = 0;
    rc = dgrad_launch(dy, wt, dx, residual, N, H, W, Cin, Cout, KH, KW, stride, pad, reinterpret_cast<float*>(static_cast<char*>(workspace) + off),
                      workspace_bytes - off, st, nullptr, img_floats > 0 ? img : nullptr, &packed);
    if (packed_route != nullptr) *packed_route = packed;
    return rc;
}

}  // extern "C"
