// What the host half (mjpeg_parse.hip: plain C++) and the device half (mjpeg_decode.hip) of the JPEG decoder share: the geometry of a
// frame and the layout of the "blob", the parsed description of one stream that travels to the device in front of its bytes.
#pragma once
#include <cstddef>
#include "jpeg_entropy.h"

constexpr int kJdMagic = 0x4a504744;       // 'JPGD'

// blob = JdBlobHead | quantiser tables [4][64] uint16, natural order | JdHuff [4]: dc0 dc1 ac0 ac1 | starts int32 [nint + 1]
// Interval i is bytes [starts[i], starts[i + 1] - 2) of the stream: every interval is followed by the two bytes of RSTm or EOI.
struct JdBlobHead {
    int magic, H, W, mode;
    int restart_mcus;            // MCUs per interval; = nmcu for a stream without DRI
    int nint, nmcu, nbytes;      // intervals, MCUs, length of the stream
    int td[3], ta[3], tq[3];     // per component: DC table, AC table (0 | 1), quantiser table (0..3)
    int has_dri, has_dht, blob_bytes;
    int pad[4];
};
static_assert(sizeof(JdBlobHead) == 96, "blob head is 24 ints");
static_assert(sizeof(JdHuff) == 1416, "JdHuff is read as dwords");
constexpr size_t kJdBlobQuant = sizeof(JdBlobHead);
constexpr size_t kJdBlobHuff = kJdBlobQuant + 4 * 64 * sizeof(unsigned short);
constexpr size_t kJdBlobStarts = kJdBlobHuff + 4 * sizeof(JdHuff);

struct JdGeom {
    int mode, ms, bpm, mcux, mcuy, nmcu, C;
    size_t nblk;
    int yh, yw, ch, cw;          // planes at MCU-padded size (ch = cw = 0 for grey)
    size_t blob_max;             // a blob with one interval per MCU, 16-byte aligned: where the stream's bytes start in a slot
    size_t coef, yoff, cboff, croff, frame;     // per-frame workspace: coefficients | Y | Cb | Cr
};

inline size_t jd_align16(size_t v) { return (v + 15) & ~(size_t)15; }

inline bool jd_geom(int H, int W, int C, int subsampling, JdGeom* g) {
    if (H < 1 || W < 1 || H > 65535 || W > 65535 || (C != 1 && C != 3)) return false;
    if (C == 3 && subsampling != 420 && subsampling != 444) return false;
    g->C = C;
    g->mode = C == 1 ? JD_MODE_GREY : (subsampling == 420 ? JD_MODE_420 : JD_MODE_444);
    g->ms = g->mode == JD_MODE_420 ? 16 : 8;
    g->bpm = g->mode == JD_MODE_420 ? 6 : (g->mode == JD_MODE_444 ? 3 : 1);
    g->mcux = (W + g->ms - 1) / g->ms;
    g->mcuy = (H + g->ms - 1) / g->ms;
    g->nmcu = g->mcux * g->mcuy;
    g->nblk = (size_t)g->nmcu * g->bpm;
    g->yh = g->mcuy * g->ms; g->yw = g->mcux * g->ms;
    g->ch = C == 1 ? 0 : g->mcuy * 8; g->cw = C == 1 ? 0 : g->mcux * 8;
    g->blob_max = jd_align16(kJdBlobStarts + ((size_t)g->nmcu + 1) * sizeof(int));
    g->coef = 0;
    g->yoff = jd_align16(g->nblk * 64 * sizeof(short));
    g->cboff = g->yoff + jd_align16((size_t)g->yh * g->yw);
    g->croff = g->cboff + jd_align16((size_t)g->ch * g->cw);
    g->frame = g->croff + jd_align16((size_t)g->ch * g->cw);
    return true;
}

// mjpeg_decode.hip: the IDCT and colour launches behind any entropy back end (stages 2 and 3 of stabnet_mjpeg_decode); a STABNET_* code
int mjpegd_launch_planes(const JdGeom& g, int H, int W, const unsigned char* in, size_t in_stride, int N, const short* coef,
                         size_t coef_stride, unsigned char* wsb, unsigned char* out, size_t row_stride, size_t frame_stride, int stages,
                         void* stream);

// mjpeg_decode.hip: the argument checks the two I420 entries share (a STABNET_* code, the sentence set), and the IDCT launch followed by
// the crop of the padded planes to the dense I420 frame (mjpegd_planes_kernel) behind any entropy back end.  prof: Prof* or null.
int mjpegd_clear_status(int* status, int N, void* stream);            // status[0..N) = 0, by a launch (see mjpeg_decode.hip)
int mjpegd_i420_geom(const char* who, int N, int H, int W, int C, int subsampling, size_t frame_stride, JdGeom* g);
int mjpegd_launch_i420(const JdGeom& g, int H, int W, const unsigned char* in, size_t in_stride, int N, const short* coef, size_t coef_stride,
                       unsigned char* wsb, unsigned char* out, size_t frame_stride, void* stream, void* prof);
