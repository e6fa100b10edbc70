// Baseline JPEG (ITU-T T.81, Huffman, 8-bit) entropy decoding of ONE restart interval, for the host and the device alike: the
// entropy kernel of mjpeg_decode.hip runs it with one lane per interval, stabnet_mjpeg_entropy_host loops it over the intervals.
// Plain C++ without library calls.  Whatever the bytes are, it reads data[pos .. end) only, writes coef[0 .. nblocks * 64) only and
// indexes every table through a mask; anything that does not decode ends the interval with a JD_* status.
#pragma once

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define JPEG_HD inline
#endif

enum { JD_MODE_GREY = 0, JD_MODE_444 = 1, JD_MODE_420 = 2 };
enum {
    JD_OK = 0,
    JD_ERR_DATA = 1,        // the interval's bytes ran out before its blocks did
    JD_ERR_CODE = 2,        // a bit pattern that is no code of the table, or a DC category above 15
    JD_ERR_INDEX = 4,       // a run that carries a coefficient past position 63
    JD_ERR_BLOB = 8,        // the parsed description does not fit the launch (geometry, offsets, table selectors)
};

constexpr int kJdLookBits = 9;

// One Huffman table as the decoder reads it (built by the parser from BITS / HUFFVAL, T.81 Annex C and F.2.2.3).
struct JdHuff {
    unsigned short look[1 << kJdLookBits];   // next 9 bits -> (length << 8) | symbol of a code of length <= 9; 0 = longer code
    int maxcode[17];                         // [l]: largest code of length l, -1 if there is none ([0] unused)
    int valoff[17];                          // [l]: index into huffval of the first code of length l, minus that code
    unsigned char huffval[256];
};

struct JdBits {
    const unsigned char* d;
    int pos, end;
    unsigned long long acc;      // the low `n` bits are unread, oldest on top
    int n, fake;                 // fake: how many of them are zeros appended behind the interval's last byte

    JPEG_HD void fill() {        // to at least 57 bits: a symbol takes at most 16 + 15
        while (n <= 56) {
            unsigned b = 0;
            if (pos < end) {
                b = d[pos++];
                if (b == 0xffu) {
                    if (pos < end && d[pos] == 0) ++pos;            // FF 00: a stuffed FF
                    else { pos = end; b = 0; fake += 8; }            // a marker (or the end): nothing behind it belongs to the interval
                }
            } else {
                fake += 8;
            }
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    JPEG_HD unsigned peek(int k) const { return (unsigned)(acc >> (n - k)) & ((1u << k) - 1u); }
    JPEG_HD bool skip(int k) { n -= k; return n >= fake; }          // false: a bit was taken that the stream does not have
};

// -> symbol 0..255, or -1 (JD_ERR_CODE) / -2 (JD_ERR_DATA).  bits.fill() must have run since the last symbol.
JPEG_HD int jd_symbol(JdBits& b, const JdHuff* h) {
    const unsigned e = h->look[b.peek(kJdLookBits)];
    if (e) return b.skip((int)(e >> 8)) ? (int)(e & 0xffu) : -2;
    for (int l = kJdLookBits + 1; l <= 16; ++l) {
        const int code = (int)b.peek(l);
        if (code <= h->maxcode[l]) return b.skip(l) ? (int)h->huffval[(h->valoff[l] + code) & 255] : -2;
    }
    return -1;
}

// T.81 F.2.2.1 EXTEND of the s-bit value v, 1 <= s <= 15
JPEG_HD int jd_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// The MCUs of one restart interval: data[pos .. end) -> coef[nmcus * bpm][64] int16 in NATURAL order, not dequantised.  coef must be
// zero on entry.  huff: the tables 0 and 1 of each class, [dc0, dc1, ac0, ac1]; td / ta: per component, 0 or 1.  DC predictors start
// at 0 (and wrap as int16, which no valid stream reaches).
JPEG_HD int jd_decode_interval(const unsigned char* data, int pos, int end, const JdHuff* huff, const int* td, const int* ta, int mode,
                               int nmcus, short* coef, const unsigned char* zigzag) {
    const int bpm = mode == JD_MODE_420 ? 6 : (mode == JD_MODE_444 ? 3 : 1);
    JdBits b;
    b.d = data; b.pos = pos; b.end = end; b.acc = 0ull; b.n = 0; b.fake = 0;
    int pred0 = 0, pred1 = 0, pred2 = 0;
    for (int m = 0; m < nmcus; ++m) {
        for (int j = 0; j < bpm; ++j) {
            const int comp = mode == JD_MODE_GREY ? 0 : (mode == JD_MODE_444 ? j : (j < 4 ? 0 : j - 3));
            const JdHuff* hd = huff + (td[comp] & 1);
            const JdHuff* ha = huff + 2 + (ta[comp] & 1);
            short* blk = coef + ((long)m * bpm + j) * 64;
            b.fill();
            int s = jd_symbol(b, hd);
            if (s < 0) return s == -1 ? JD_ERR_CODE : JD_ERR_DATA;
            if (s > 15) return JD_ERR_CODE;
            int diff = 0;
            if (s) {
                diff = jd_extend((int)b.peek(s), s);
                if (!b.skip(s)) return JD_ERR_DATA;
            }
            const int dc = (int)(short)((comp == 0 ? pred0 : (comp == 1 ? pred1 : pred2)) + diff);
            if (comp == 0) pred0 = dc; else if (comp == 1) pred1 = dc; else pred2 = dc;
            blk[0] = (short)dc;
            int k = 1;
            while (k < 64) {
                b.fill();
                const int rs = jd_symbol(b, ha);
                if (rs < 0) return rs == -1 ? JD_ERR_CODE : JD_ERR_DATA;
                const int r = rs >> 4;
                s = rs & 15;
                if (s == 0) {
                    if (r != 15) break;              // EOB
                    k += 16;                         // ZRL
                    continue;
                }
                k += r;
                if (k > 63) return JD_ERR_INDEX;
                const int v = jd_extend((int)b.peek(s), s);
                if (!b.skip(s)) return JD_ERR_DATA;
                blk[zigzag[k]] = (short)v;
                ++k;
            }
        }
    }
    return JD_OK;
}
