// Host half of the JPEG decoder: plain C++ (no HIP call, no device code; it also compiles as C++ on its own for the sanitizer
// program of tests/mjpeg_decode_fuzz_main.cpp).  stabnet_mjpeg_parse reads the marker segments of one baseline stream, finds its
// restart intervals (FF D0..D7 inside scan data is always a marker: a linear scan of bytes that are on the host anyway) and packs
// what the kernels of mjpeg_decode.hip read into a blob (mjpeg_decode.h); stabnet_mjpeg_entropy_host decodes the coefficients on the
// CPU with the routine the entropy kernel runs (jpeg_entropy.h), for streams without DRI: one interval, one sequential decode.
// stabnet_mjpeg_entropy_sync_host is the host twin of mjpeg_decode_sync.hip, which does decode such an interval in parallel: the
// phases of jpeg_sync.h with the lanes in a loop, for tests (tests/mjpeg_sync_fuzz_main.cpp runs it under the sanitizers).
#include <cstdint>
#include <cstring>
#include <vector>
#include "jpeg_sync.h"
#include "jpeg_tables.h"
#include "mjpeg_decode.h"

void stabnet_set_error(const char* fmt, ...);

#define STABNET_MJPEG_UNSUPPORTED 1

namespace {

// BITS / HUFFVAL -> what jd_symbol reads.  false: more than 256 symbols, or more codes of a length than that length has.
bool jd_build_huff(const unsigned char* bits16, const unsigned char* vals, int nvals, bool dc, JdHuff* h) {
    memset(h, 0, sizeof(*h));
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = bits16[l - 1];
        h->maxcode[l] = -1;
        h->valoff[l] = k - code;
        if (cnt) {
            if (k + cnt > nvals || code + cnt > (1 << l)) return false;
            for (int i = 0; i < cnt; ++i, ++k, ++code) {
                if (dc && vals[k] > 15) return false;
                h->huffval[k] = vals[k];
                if (l <= kJdLookBits) {
                    const int lo = code << (kJdLookBits - l);
                    for (int f = 0; f < (1 << (kJdLookBits - l)); ++f) h->look[lo + f] = (unsigned short)((l << 8) | vals[k]);
                }
            }
            h->maxcode[l] = code - 1;
        }
        code <<= 1;
    }
    return true;
}

struct Rd {
    const unsigned char* p;
    size_t n, i;
    bool has(size_t k) const { return i + k <= n; }
    int u8() { return p[i++]; }
    int u16() { const int v = (p[i] << 8) | p[i + 1]; i += 2; return v; }
};

}  // namespace

extern "C" {

/* See include/stabnet_hip.h. */
size_t stabnet_mjpeg_decode_blob_bytes(int H, int W, int C, int subsampling) {
    JdGeom g;
    if (!jd_geom(H, W, C, subsampling, &g)) {
        stabnet_set_error("mjpeg_decode_blob_bytes: bad shape, channels or subsampling");
        return 0;
    }
    return g.blob_max;
}

int stabnet_mjpeg_parse(const unsigned char* jpeg, size_t nbytes, int* info16, unsigned char* blob, size_t blob_cap) {
    if (!jpeg || !info16) { stabnet_set_error("mjpeg_parse: null pointer"); return -1; }
    memset(info16, 0, 16 * sizeof(int));
    if (nbytes < 4 || nbytes >= ((size_t)1 << 30)) { stabnet_set_error("mjpeg_parse: %zu bytes is no JPEG stream", nbytes); return -1; }
#define JD_CORRUPT(...) do { stabnet_set_error("mjpeg_parse: " __VA_ARGS__); return -1; } while (0)
#define JD_UNSUPPORTED(...) do { stabnet_set_error("mjpeg_parse: unsupported: " __VA_ARGS__); return STABNET_MJPEG_UNSUPPORTED; } while (0)
    Rd r{jpeg, nbytes, 0};
    if (r.u16() != 0xffd8) JD_CORRUPT("no SOI");
    unsigned short quant[4][64];
    bool have_q[4] = {false, false, false, false};
    JdHuff huff[4];
    for (int t = 0; t < 2; ++t) {                       // a stream without DHT is coded with the Annex K tables
        jd_build_huff(kDcBits[t], kDcVals, 12, true, &huff[t]);
        jd_build_huff(kAcBits[t], kAcVals[t], 162, false, &huff[2 + t]);
    }
    memset(quant, 0, sizeof(quant));
    int H = 0, W = 0, C = 0, restart = 0, has_dri = 0, has_dht = 0;
    int cid[3] = {0, 0, 0}, hv[3] = {0, 0, 0}, tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    bool have_sof = false;
    size_t scan = 0;
    while (!scan) {
        if (!r.has(2)) JD_CORRUPT("the stream ends before SOS");
        if (r.u8() != 0xff) JD_CORRUPT("marker expected at byte %zu", r.i - 1);
        int m = r.u8();
        while (m == 0xff && r.has(1)) m = r.u8();        // fill bytes
        if (m == 0xd8 || m == 0x01 || (m >= 0xd0 && m <= 0xd7)) continue;     // no segment
        if (m == 0xd9) JD_CORRUPT("EOI before SOS");
        if (!r.has(2)) JD_CORRUPT("the stream ends inside a segment");
        const int len = r.u16();
        if (len < 2 || !r.has((size_t)len - 2)) JD_CORRUPT("segment %02x of %d bytes runs past the end", m, len);
        Rd s{jpeg, r.i + (size_t)len - 2, r.i};
        r.i += (size_t)len - 2;
        if (m == 0xdb) {
            while (s.has(1)) {
                const int pt = s.u8();
                if (pt >> 4) JD_UNSUPPORTED("16-bit quantiser table");
                if ((pt & 15) > 3 || !s.has(64)) JD_CORRUPT("bad DQT");
                for (int z = 0; z < 64; ++z) quant[pt & 15][kZigzag[z]] = (unsigned short)s.u8();
                have_q[pt & 15] = true;
            }
        } else if (m == 0xc0) {
            if (have_sof || !s.has(6)) JD_CORRUPT("bad SOF0");
            const int prec = s.u8();
            H = s.u16(); W = s.u16(); C = s.u8();
            if (prec != 8) JD_UNSUPPORTED("%d-bit samples", prec);
            if (C != 1 && C != 3) JD_UNSUPPORTED("%d components", C);
            if (H < 1 || W < 1 || !s.has((size_t)3 * C)) JD_CORRUPT("bad SOF0");
            for (int c = 0; c < C; ++c) { cid[c] = s.u8(); hv[c] = s.u8(); tq[c] = s.u8(); }
            have_sof = true;
        } else if ((m >= 0xc1 && m <= 0xcf) && m != 0xc4 && m != 0xc8 && m != 0xcc) {
            JD_UNSUPPORTED("SOF%d (only baseline, SOF0, is decoded)", m - 0xc0);
        } else if (m == 0xcc) {
            JD_UNSUPPORTED("arithmetic coding");
        } else if (m == 0xc4) {
            has_dht = 1;
            while (s.has(1)) {
                const int tc = s.u8();
                if ((tc >> 4) > 1 || !s.has(16)) JD_CORRUPT("bad DHT");
                if ((tc & 15) > 1) JD_UNSUPPORTED("Huffman table %d (baseline has 0 and 1)", tc & 15);
                const unsigned char* bits = jpeg + s.i;
                int cnt = 0;
                for (int i = 0; i < 16; ++i) cnt += s.u8();
                if (cnt > 256 || !s.has((size_t)cnt)) JD_CORRUPT("bad DHT");
                if (!jd_build_huff(bits, jpeg + s.i, cnt, (tc >> 4) == 0, &huff[(tc >> 4) * 2 + (tc & 15)])) JD_CORRUPT("DHT is no Huffman code");
                s.i += (size_t)cnt;
            }
        } else if (m == 0xdd) {
            if (!s.has(2)) JD_CORRUPT("bad DRI");
            restart = s.u16();
            has_dri = restart > 0;
        } else if (m == 0xee) {
            if (len >= 14 && memcmp(jpeg + s.i, "Adobe", 5) == 0) JD_UNSUPPORTED("Adobe colour transform marker");
        } else if (m == 0xda) {
            if (!have_sof) JD_CORRUPT("SOS before SOF0");
            if (!s.has(1)) JD_CORRUPT("bad SOS");
            const int ns = s.u8();
            if (ns != C) JD_UNSUPPORTED("a scan of %d of %d components (multiple scans)", ns, C);
            if (!s.has((size_t)2 * ns + 3)) JD_CORRUPT("bad SOS");
            for (int c = 0; c < ns; ++c) {
                const int id = s.u8(), t = s.u8();
                if (id != cid[c]) JD_UNSUPPORTED("scan components out of frame order");
                td[c] = t >> 4; ta[c] = t & 15;
                if (td[c] > 1 || ta[c] > 1) JD_UNSUPPORTED("Huffman table above 1");
            }
            const int ss = s.u8(), se = s.u8(), ahl = s.u8();
            if (ss != 0 || se != 63 || ahl != 0) JD_UNSUPPORTED("spectral selection / successive approximation");
            scan = r.i;
        }
        /* APPn, COM and anything else with a length: skipped */
    }
    int sub = 0;
    if (C == 1) {
        if (hv[0] != 0x11) JD_UNSUPPORTED("grey sampled %02x", hv[0]);
    } else {
        if (cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B') JD_UNSUPPORTED("RGB components");
        if (hv[1] != 0x11 || hv[2] != 0x11 || (hv[0] != 0x22 && hv[0] != 0x11))
            JD_UNSUPPORTED("sampling %02x %02x %02x (4:2:0 and 4:4:4 are decoded)", hv[0], hv[1], hv[2]);
        sub = hv[0] == 0x22 ? 420 : 444;
    }
    for (int c = 0; c < C; ++c)
        if (tq[c] > 3 || !have_q[tq[c]]) JD_CORRUPT("component %d uses quantiser table %d, which the stream does not define", c, tq[c]);
    JdGeom g;
    if (!jd_geom(H, W, C, sub, &g)) JD_CORRUPT("bad size %dx%d", W, H);
    const int R = has_dri ? (restart < g.nmcu ? restart : g.nmcu) : g.nmcu;
    const int nint = (g.nmcu + R - 1) / R;
    const size_t blob_bytes = jd_align16(kJdBlobStarts + ((size_t)nint + 1) * sizeof(int));
    const bool write = blob != nullptr;
    if (write && blob_cap < blob_bytes) { stabnet_set_error("mjpeg_parse: blob needs %zu bytes, cap is %zu", blob_bytes, blob_cap); return -1; }
    int* starts = write ? reinterpret_cast<int*>(blob + kJdBlobStarts) : nullptr;
    if (write && ((uintptr_t)blob & 3)) { stabnet_set_error("mjpeg_parse: blob must be 4-byte aligned"); return -1; }
    // the scan: FF 00 is data, FF FF fill, FF D0..D7 ends an interval, anything else ends the scan
    int found = 0;
    size_t i = scan, end = 0;
    if (write) starts[0] = (int)scan;
    while (i + 1 < nbytes) {
        if (jpeg[i] != 0xff) { ++i; continue; }
        const int m = jpeg[i + 1];
        if (m == 0x00) { i += 2; continue; }
        if (m == 0xff) { ++i; continue; }
        if (m >= 0xd0 && m <= 0xd7) {
            if (m != 0xd0 + (found & 7)) JD_UNSUPPORTED("restart markers out of sequence");
            ++found;
            if (found >= nint) JD_UNSUPPORTED("more restart markers than DRI %d gives for %d MCUs", restart, g.nmcu);
            i += 2;
            if (write) starts[found] = (int)i;
            continue;
        }
        if (m != 0xd9) JD_UNSUPPORTED("marker %02x after the scan (multiple scans)", m);
        end = i;
        break;
    }
    if (!end) JD_CORRUPT("the stream ends without EOI");
    if (found != nint - 1) JD_UNSUPPORTED("%d restart markers, DRI %d gives %d for %d MCUs", found, restart, nint - 1, g.nmcu);
    if (write) {
        starts[nint] = (int)end + 2;
        JdBlobHead h;
        memset(&h, 0, sizeof(h));
        h.magic = kJdMagic; h.H = H; h.W = W; h.mode = g.mode; h.restart_mcus = R; h.nint = nint; h.nmcu = g.nmcu; h.nbytes = (int)nbytes;
        for (int c = 0; c < 3; ++c) { h.td[c] = td[c]; h.ta[c] = ta[c]; h.tq[c] = tq[c]; }
        h.has_dri = has_dri; h.has_dht = has_dht; h.blob_bytes = (int)blob_bytes;
        memcpy(blob, &h, sizeof(h));
        memcpy(blob + kJdBlobQuant, quant, sizeof(quant));
        memcpy(blob + kJdBlobHuff, huff, sizeof(huff));
    }
    info16[0] = H; info16[1] = W; info16[2] = C; info16[3] = sub; info16[4] = has_dri ? restart : 0; info16[5] = nint; info16[6] = g.nmcu;
    info16[7] = (int)scan; info16[8] = (int)end; info16[9] = (int)blob_bytes; info16[10] = has_dht; info16[11] = (int)g.nblk;
    return 0;
#undef JD_CORRUPT
#undef JD_UNSUPPORTED
}

int stabnet_mjpeg_entropy_host(const unsigned char* jpeg, size_t nbytes, const unsigned char* blob, size_t blob_bytes, short* coef,
                               size_t coef_count) {
    if (!jpeg || !blob || !coef) { stabnet_set_error("mjpeg_entropy_host: null pointer"); return -1; }
    if (blob_bytes < kJdBlobStarts + 2 * sizeof(int) || ((uintptr_t)blob & 3)) { stabnet_set_error("mjpeg_entropy_host: bad blob"); return -1; }
    JdBlobHead h;
    memcpy(&h, blob, sizeof(h));
    JdGeom g;
    const int C = h.mode == JD_MODE_GREY ? 1 : 3;
    if (h.magic != kJdMagic || h.mode < 0 || h.mode > 2 || !jd_geom(h.H, h.W, C, h.mode == JD_MODE_420 ? 420 : 444, &g) || h.nmcu != g.nmcu ||
        h.restart_mcus < 1 || h.nint != (g.nmcu + h.restart_mcus - 1) / h.restart_mcus || (size_t)h.nbytes != nbytes ||
        blob_bytes < kJdBlobStarts + ((size_t)h.nint + 1) * sizeof(int)) {
        stabnet_set_error("mjpeg_entropy_host: the blob is not stabnet_mjpeg_parse's for this stream");
        return -1;
    }
    if (coef_count < g.nblk * 64) { stabnet_set_error("mjpeg_entropy_host: %zu coefficients, the frame has %zu", coef_count, g.nblk * 64); return -1; }
    memset(coef, 0, g.nblk * 64 * sizeof(short));
    const JdHuff* huff = reinterpret_cast<const JdHuff*>(blob + kJdBlobHuff);
    const int* starts = reinterpret_cast<const int*>(blob + kJdBlobStarts);
    int status = 0;
    for (int it = 0; it < h.nint; ++it) {
        const long a = starts[it], b = (long)starts[it + 1] - 2;
        if (a < 0 || b < a || (size_t)b > nbytes) { status |= JD_ERR_BLOB; continue; }
        const int m0 = it * h.restart_mcus, m1 = m0 + h.restart_mcus < g.nmcu ? m0 + h.restart_mcus : g.nmcu;
        status |= jd_decode_interval(jpeg, (int)a, (int)b, huff, h.td, h.ta, h.mode, m1 - m0, coef + (size_t)m0 * g.bpm * 64, kZigzag);
    }
    if (status) {
        stabnet_set_error("mjpeg_entropy_host: the scan does not decode (status %d: 1 data ran out, 2 no such code, 4 run past 63, 8 offsets)", status);
        return -1;
    }
    return 0;
}

/* The phases of mjpeg_decode_sync.hip with the lanes in a loop: guess, rounds inside groups of kGroup chunks, one hand-over across
 * the groups and the rounds again, verify, repair, scan, write.  See include/stabnet_hip.h. */
int stabnet_mjpeg_entropy_sync_host(const unsigned char* jpeg, size_t nbytes, const unsigned char* blob, size_t blob_bytes, short* coef,
                                    size_t coef_count, int chunk_bytes, int rounds, int* stats) {
    constexpr int kGroup = 256;
    if (!jpeg || !blob || !coef) { stabnet_set_error("mjpeg_entropy_sync_host: null pointer"); return -1; }
    if (chunk_bytes < 1 || chunk_bytes > (1 << 20)) { stabnet_set_error("mjpeg_entropy_sync_host: chunk_bytes %d is not in 1..2^20", chunk_bytes); return -1; }
    if (blob_bytes < kJdBlobStarts + 2 * sizeof(int) || ((uintptr_t)blob & 3)) { stabnet_set_error("mjpeg_entropy_sync_host: bad blob"); return -1; }
    if (rounds < 0) rounds = kJsDefaultRounds;
    JdBlobHead h;
    memcpy(&h, blob, sizeof(h));
    JdGeom g;
    const int C = h.mode == JD_MODE_GREY ? 1 : 3;
    if (h.magic != kJdMagic || h.mode < 0 || h.mode > 2 || !jd_geom(h.H, h.W, C, h.mode == JD_MODE_420 ? 420 : 444, &g) || h.nmcu != g.nmcu ||
        (size_t)h.nbytes != nbytes) {
        stabnet_set_error("mjpeg_entropy_sync_host: the blob is not stabnet_mjpeg_parse's for this stream");
        return -1;
    }
    if (h.nint != 1 || h.restart_mcus != g.nmcu) {
        stabnet_set_error("mjpeg_entropy_sync_host: the stream has %d restart intervals; this back end decodes streams of one (status 8)", h.nint);
        return -1;
    }
    if (coef_count < g.nblk * 64) { stabnet_set_error("mjpeg_entropy_sync_host: %zu coefficients, the frame has %zu", coef_count, g.nblk * 64); return -1; }
    memset(coef, 0, g.nblk * 64 * sizeof(short));
    const JdHuff* huff = reinterpret_cast<const JdHuff*>(blob + kJdBlobHuff);
    const int* starts = reinterpret_cast<const int*>(blob + kJdBlobStarts);
    const long a = starts[0], b = (long)starts[1] - 2;
    if (a < 0 || b < a || (size_t)b > nbytes) { stabnet_set_error("mjpeg_entropy_sync_host: the scan does not decode (status 8: offsets)"); return -1; }
    const int nc = js_nchunks((int)a, (int)b, chunk_bytes);
    std::vector<JsState> entry((size_t)nc), exits((size_t)nc), old;
    std::vector<JsSum> sums((size_t)nc);
    auto walk = [&](int c) {
        js_walk<false>(jpeg, (int)b, js_limit(c, nc, (int)a, chunk_bytes), entry[c], huff, h.td, h.ta, h.mode, &exits[c], &sums[c], 0, 0, 0u, 0u,
                       0u, nullptr, kZigzag);
    };
    for (int c = 0; c < nc; ++c) {                        // 1. guess
        entry[c] = js_guess(jpeg, (int)a, (int)b, c, chunk_bytes);
        walk(c);
    }
    for (int pass = 0; pass < (rounds > 0 ? 2 : 0); ++pass) {       // 2. synchronise: inside the groups, then once across them
        for (int r = 0; r < rounds; ++r) {
            old = exits;
            bool any = false;
            for (int c = 1; c < nc; ++c) {
                if (c % kGroup == 0 && (pass == 0 || r > 0)) continue;
                if (js_same(old[c - 1], entry[c])) continue;
                entry[c] = old[c - 1];
                walk(c);
                any = true;
            }
            if (!any) break;
        }
    }
    int repaired = 0;                                      // 3. verify and repair, left to right
    for (int c = 1; c < nc; ++c) {
        if (js_same(exits[c - 1], entry[c])) continue;
        entry[c] = exits[c - 1];
        walk(c);
        ++repaired;
    }
    if (stats) { stats[0] = nc; stats[1] = nc - repaired; }
    JsSum run = {0u, 0u, 0u, 0u};                          // 4. count, scan, write (the DC sums ride along: 5.)
    int status = 0;
    for (int c = 0; c < nc; ++c) {
        JsState ex;
        JsSum s;
        status |= js_walk<true>(jpeg, (int)b, js_limit(c, nc, (int)a, chunk_bytes), entry[c], huff, h.td, h.ta, h.mode, &ex, &s, (long)run.cnt - 1,
                                (long)g.nblk, run.dc0, run.dc1, run.dc2, coef, kZigzag);
        js_add(run, s);
    }
    if ((size_t)run.cnt < g.nblk) status |= JD_ERR_DATA;
    if (status) {
        stabnet_set_error("mjpeg_entropy_sync_host: the scan does not decode (status %d: 1 data ran out, 2 no such code, 4 run past 63, 8 offsets)", status);
        return -1;
    }
    return 0;
}

}  // extern "C"
