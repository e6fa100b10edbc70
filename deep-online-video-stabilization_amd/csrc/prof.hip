// The Profiler ABI (include/stabnet_hip.h): records of HIP-event pairs around launches (prof.h) and the kernel name of every record kind.
#include "conv.h"
#include "prof.h"
#include "../../include/stabnet_hip.h"   // (a check of this file's entries against their declarations)

extern "C" {

int stabnet_prof_create(void** out, int max_records) {
    SN_REQUIRE(out && max_records > 0 && max_records <= (1 << 20), "prof_create: bad arguments");
    Prof* p = new Prof();
    p->cap = max_records;
    p->ev.resize(2 * (size_t)max_records);
    p->kind.resize(max_records); p->flops.resize(max_records); p->bytes.resize(max_records);
    p->shape.resize(4 * (size_t)max_records);
    for (auto& e : p->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            stabnet_set_error("prof_create: hipEventCreate failed");
            return STABNET_ERR_LAUNCH;
        }
    *out = p;
    return STABNET_OK;
}
void stabnet_prof_destroy(void* pp) {
    Prof* p = static_cast<Prof*>(pp);
    if (!p) return;
    for (auto& e : p->ev) (void)hipEventDestroy(e);
    delete p;
}
int stabnet_prof_reset(void* pp) {
    SN_REQUIRE(pp, "prof_reset: null");
    static_cast<Prof*>(pp)->n = 0;
    return STABNET_OK;
}
/* Records one event pair with nothing between them on `stream` (kind 0): the per-pair overhead to subtract. */
int stabnet_prof_record_empty(void* pp, void* stream) {
    Prof* p = static_cast<Prof*>(pp);
    SN_REQUIRE(p, "prof_record_empty: null");
    if (p->begin((hipStream_t)stream)) p->end((hipStream_t)stream, 0, 0.0, 0.0);
    return STABNET_OK;
}
int stabnet_prof_num_records(const void* pp) { return pp ? static_cast<const Prof*>(pp)->n : -1; }
/* The stream the records were taken on must have been synchronised by the caller. */
int stabnet_prof_record(const void* pp, int idx, int* kind, float* ms, double* flops, double* bytes) {
    const Prof* p = static_cast<const Prof*>(pp);
    SN_REQUIRE(p && idx >= 0 && idx < p->n && kind && ms && flops && bytes, "prof_record: bad arguments");
    hipError_t e = hipEventElapsedTime(ms, p->ev[2 * idx], p->ev[2 * idx + 1]);
    if (e != hipSuccess) {
        stabnet_set_error("prof_record: %s", hipGetErrorString(e));
        return STABNET_ERR_LAUNCH;
    }
    *kind = p->kind[idx]; *flops = p->flops[idx]; *bytes = p->bytes[idx];
    return STABNET_OK;
}
/* GEMM view of a record: shape4 = {M, N, K, split-K}; zeros for non-GEMM kernels. */
int stabnet_prof_record_shape(const void* pp, int idx, int* shape4) {
    const Prof* p = static_cast<const Prof*>(pp);
    SN_REQUIRE(p && idx >= 0 && idx < p->n && shape4, "prof_record_shape: bad arguments");
    for (int i = 0; i < 4; ++i) shape4[i] = p->shape[4 * idx + i];
    return STABNET_OK;
}
const char* stabnet_prof_kind_name(int kind) {
    switch (kind) {
        case PK_KERNEL_PAD: return "pad_channels_kernel";
        case PK_KERNEL_POOL: return "max_pool_kernel";
        case PK_KERNEL_GAP: return "gap_bn_relu_partial_kernel";
        case PK_KERNEL_FC: return "fc_kernel";
        case PK_KERNEL_MESH: return "mesh_homography_kernel";
        case PK_KERNEL_HEAD: return "theta_mesh_kernel";
        case PK_KERNEL_WARP: return "warp_sample_kernel";
        case PK_KERNEL_ASSEMBLE: return "stack_assemble_bordered_kernel";
        case PK_KERNEL_PUSH: return "ring_push_kernel";
        case PK_KERNEL_SPLITK_REDUCE: return "conv_splitk_reduce_kernel";
        case PK_KERNEL_WGRAD: return "conv_wgrad_f32_kernel";
        case PK_KERNEL_MJPEG_TRANSFORM: return "mjpeg_transform_kernel";
        case PK_KERNEL_MJPEG_ENTROPY: return "mjpeg_entropy_kernel";
        case PK_KERNEL_MJPEG_LAYOUT: return "mjpeg_layout_kernel";
        case PK_KERNEL_MJPEG_GATHER: return "mjpeg_gather_kernel";
        case PK_KERNEL_INGEST_GREY_ROWS: return "ingest_grey_rows_kernel";
        case PK_KERNEL_INGEST_GREY_COLS: return "ingest_grey_cols_kernel";
        case PK_KERNEL_INGEST_COLOUR: return "ingest_colour_kernel";
        case PK_KERNEL_MAP_SHRINK: return "map_shrink_kernel";
        case PK_KERNEL_REMAP_SRC: return "remap_src_kernel";
        case PK_KERNEL_REMAP_SRC4: return "remap_src4_kernel";
        case PK_KERNEL_REMAP_WIN: return "remap_win_kernel";
        case PK_KERNEL_REMAP_WIN4: return "remap_win4_kernel";
        case PK_KERNEL_REMAP_WIN_DEV: return "remap_win_dev_kernel";
        case PK_KERNEL_REMAP_WIN4_DEV: return "remap_win4_dev_kernel";
        case PK_KERNEL_REMAP_I420: return "remap_i420_kernel";
        case PK_KERNEL_REMAP_CUBIC + 0: return "remap_cubic_kernel<1, 0>";
        case PK_KERNEL_REMAP_CUBIC + 1: return "remap_cubic_kernel<4, 0>";
        case PK_KERNEL_REMAP_CUBIC + 2: return "remap_cubic_kernel<1, 1>";
        case PK_KERNEL_REMAP_CUBIC + 3: return "remap_cubic_kernel<4, 1>";
        case PK_KERNEL_REMAP_CUBIC + 4: return "remap_cubic_kernel<1, 2>";
        case PK_KERNEL_REMAP_CUBIC + 5: return "remap_cubic_kernel<4, 2>";
        case PK_KERNEL_REMAP_I420_CUBIC: return "remap_i420_kernel<true>";
        case PK_KERNEL_MJPEGD_PLANES: return "mjpegd_planes_kernel";
        case PK_KERNEL_MJPEG_TRANSFORM_PLANAR: return "mjpeg_transform_planar_kernel";
        case PK_KERNEL_TF_GET_IMG: return "tf_get_img_kernel";
        case PK_KERNEL_TVL1_STEP: return "tvl1_step_kernel";
        case PK_KERNEL_TVL1_FUSED: return "tvl1_fused_kernel";
        case PK_KERNEL_TVL1_DOWN: return "tvl1_down_kernel";
        case PK_KERNEL_TVL1_GRAD: return "tvl1_grad_kernel";
        case PK_KERNEL_TVL1_WARP: return "tvl1_warp_kernel";
        case PK_KERNEL_TVL1_UP: return "tvl1_up_kernel";
        case PK_KERNEL_TVL1_MAP: return "tvl1_map_kernel";
        case PK_KERNEL_KLT_DETECT: return "klt_detect_kernel";
        case PK_KERNEL_KLT_TRACK: return "klt_track_kernel";
        case PK_KERNEL_KLT_FINISH: return "klt_finish_kernel";
        case PK_KERNEL_HOMFIT: return "homfit_kernel";
        default: break;
    }
    if (kind >= PK_KERNEL_WGRAD_SAME && kind < PK_KERNEL_WGRAD_SAME + 6) {      // names as rocprofv3 prints them: <K3, PRO, BIAS>
        static const char* const names[6] = {"conv_wgrad_same_f32_kernel<0, 0, 0>", "conv_wgrad_same_f32_kernel<0, 1, 0>",
                                             "conv_wgrad_same_f32_kernel<1, 0, 0>", "conv_wgrad_same_f32_kernel<1, 1, 0>",
                                             "conv_wgrad_same_f32_kernel<0, 0, 1>", "conv_wgrad_same_f32_kernel<0, 1, 1>"};
        return names[kind - PK_KERNEL_WGRAD_SAME];
    }
    const char* conv = conv_prof_kind_name(kind);              // the PK_KERNEL_CONV_* kinds: named where they are numbered (conv.hip)
    if (conv != nullptr) return conv;
    return "?";
}

}  // extern "C"
