// Self-synchronising parallel Huffman decoding of ONE restart interval (Klein & Wiseman; Weissenberger & Schmidt), for the device
// (mjpeg_decode_sync.hip: one lane per chunk) and the host twin (stabnet_mjpeg_entropy_sync_host: the same phases, the "lanes" in a
// loop) alike.  Plain C++ without library calls.  The interval's bytes [a, b) are cut into chunks of `chunk` bytes; chunk c is
// [a + c chunk, a + (c + 1) chunk), the last one open-ended.
//   state   where a symbol starts: (byte, bit) in the stuffed stream, block-in-MCU j, zig-zag index k (0: a DC symbol comes next).
//           A position never rests on the stuffed 00 of FF 00.  DC predictors and block ordinals are NOT part of it: chunks carry
//           their count of started blocks and their per-component sum of DC differences instead, and an exclusive scan over the
//           chunks gives every chunk its first block ordinal and its predictors.
//   walk    js_walk(chunk, entry) decodes the symbols that START inside the chunk and returns the first state at or behind the
//           chunk's end (an entry already behind it passes through).  It is ONE deterministic function of (chunk, entry) in every
//           phase: a pattern that is no code, or a run past 63, ends the block and goes on with the next one (so a walk from a
//           guessed state finds its way back); bits taken behind the interval's end kill the walk (JS_DEAD, which every later
//           chunk passes on).  Every step consumes at least one bit.
//   chain   entry[c] is accepted only if it IS exit[c - 1] (a guess carries JS_GUESS and equals no exit); entry[0] is the interval's
//           start.  By induction a chain of accepted entries is the sequential decode, whatever the stream does.
// Whatever the bytes are, a walk reads data[entry .. end) only, writes coef[0 .. nblk * 64) only and masks table indices.  With
// WRITE, blocks at or beyond nblk are dropped together with their errors (the padding behind the last block decodes to anything).
#pragma once
#include "jpeg_entropy.h"

enum { JS_GUESS = 1 << 16, JS_DEAD = 1 << 17 };
constexpr int kJsNoLimit = 0x7fffffff;
constexpr int kJsDefaultChunk = 64, kJsDefaultRounds = 8;

struct JsState { int pos, meta; };                   // meta: bit | j << 3 | k << 6 | JS_GUESS | JS_DEAD
struct JsSum { unsigned cnt, dc0, dc1, dc2; };       // blocks started; DC differences per component (they wrap, like the predictors)

JPEG_HD bool js_same(JsState a, JsState b) { return a.pos == b.pos && a.meta == b.meta; }
JPEG_HD int js_nchunks(int a, int b, int chunk) { const long n = ((long)b - a + chunk - 1) / chunk; return n < 1 ? 1 : (int)n; }
JPEG_HD int js_limit(int c, int nc, int a, int chunk) { return c >= nc - 1 ? kJsNoLimit : (int)((long)a + ((long)c + 1) * chunk); }
JPEG_HD void js_add(JsSum& t, const JsSum& s) { t.cnt += s.cnt; t.dc0 += s.dc0; t.dc1 += s.dc1; t.dc2 += s.dc2; }

// JdBits that knows where its next unread bit lies: lp counts the stream bytes behind the loads (two for FF 00, one for each zero
// byte made up behind the end), ff marks the loads that were an FF 00.
struct JsBits : JdBits {
    int lp;
    unsigned ff;

    JPEG_HD void open(const unsigned char* data, int p, int e, int bit) {
        d = data; end = e; pos = p < e ? p : e; lp = pos; acc = 0ull; n = 0; fake = 0; ff = 0u;
        fill();
        n -= bit;
    }
    JPEG_HD void fill() {
        while (n <= 56) {
            unsigned b = 0;
            ff <<= 1;
            ++lp;
            if (pos < end) {
                b = d[pos++];
                if (b == 0xffu) {
                    if (pos < end && d[pos] == 0) { ++pos; ++lp; ff |= 1u; }
                    else { pos = end; b = 0; fake += 8; }
                }
            } else {
                fake += 8;
            }
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    JPEG_HD void where(int* byte, int* bit) const {
        const int u = (n + 7) >> 3;                  // loads not used up, the one in use included: at most 8
        *byte = lp - u - __builtin_popcount(ff & ((1u << u) - 1u));
        *bit = (-n) & 7;
    }
};

// jd_symbol for lanes that run in lockstep: a code longer than the look-up's 9 bits is found by testing the lengths 10..16 side by
// side (independent loads, no early exit) instead of one after the other -- in a wave of 64 walks some lane meets a long code at
// nearly every step, and the others wait for its loop.  The smallest length that fits is the one the sequential loop finds first.
JPEG_HD int js_symbol(JdBits& b, const JdHuff* h) {
    const unsigned e = h->look[b.peek(kJdLookBits)];
    if (e) return b.skip((int)(e >> 8)) ? (int)(e & 0xffu) : -2;
    const int c16 = (int)b.peek(16);
    int l = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int t = 16; t > kJdLookBits; --t)
        if ((c16 >> (16 - t)) <= h->maxcode[t]) l = t;
    if (!l) return -1;
    return b.skip(l) ? (int)h->huffval[(h->valoff[l] + (c16 >> (16 - l))) & 255] : -2;
}

// The state a lane guesses for chunk c >= 1 (c < nchunks): its first byte (one later when that is a stuffed 00), a DC symbol of
// block 0 next.  Chunk 0 starts from the truth.
JPEG_HD JsState js_guess(const unsigned char* data, int a, int b, int c, int chunk) {
    JsState s;
    s.pos = a; s.meta = 0;
    if (c <= 0) return s;
    long p = (long)a + (long)c * chunk;
    if (p >= b) p = b;
    else if (data[p - 1] == 0xffu && data[p] == 0) ++p;
    s.pos = (int)p; s.meta = JS_GUESS;
    return s;
}

// -> JD_* bits met in blocks below nblk (WRITE only; 0 otherwise).  limit: the chunk's end (kJsNoLimit for the last chunk).  sum: what
// the chunk adds.  WRITE: blk = the ordinal of the last block started in front of the chunk (-1: none), pred = the predictors there,
// coef zero on entry.
template <bool WRITE>
JPEG_HD int js_walk(const unsigned char* data, int end, int limit, JsState in, const JdHuff* huff, const int* td, const int* ta, int mode,
                    JsState* out, JsSum* sum, long blk, long nblk, unsigned pred0, unsigned pred1, unsigned pred2, short* coef,
                    const unsigned char* zigzag) {
    const int bpm = mode == JD_MODE_420 ? 6 : (mode == JD_MODE_444 ? 3 : 1);
    sum->cnt = 0u; sum->dc0 = 0u; sum->dc1 = 0u; sum->dc2 = 0u;
    out->pos = in.pos; out->meta = in.meta & ~JS_GUESS;
    if ((in.meta & JS_DEAD) || in.pos >= limit) return 0;
    int j = (in.meta >> 3) & 7, k = (in.meta >> 6) & 63;
    if (j >= bpm) j = 0;
    JsBits b;
    b.open(data, in.pos, end, in.meta & 7);
    int err = 0;
    for (;;) {
        b.fill();
        int byte, bit;
        b.where(&byte, &bit);
        if (byte >= limit) {
            out->pos = byte; out->meta = bit | (j << 3) | (k << 6);
            return err;
        }
        const int comp = mode == JD_MODE_GREY ? 0 : (mode == JD_MODE_444 ? j : (j < 4 ? 0 : j - 3));
        int e = 0;
        bool done = false;                           // the block ends here
        if (k == 0) {
            ++sum->cnt;
            ++blk;
            const int s = js_symbol(b, huff + (td[comp] & 1));
            if (s == -2) e = JD_ERR_DATA;
            else if (s == -1) e = b.skip(1) ? JD_ERR_CODE : JD_ERR_DATA;
            else if (s > 15) e = JD_ERR_CODE;
            else {
                int diff = 0;
                if (s) {
                    diff = jd_extend((int)b.peek(s), s);
                    if (!b.skip(s)) e = JD_ERR_DATA;
                }
                if (!e) {
                    unsigned p;
                    if (comp == 0) { sum->dc0 += (unsigned)diff; p = pred0 += (unsigned)diff; }
                    else if (comp == 1) { sum->dc1 += (unsigned)diff; p = pred1 += (unsigned)diff; }
                    else { sum->dc2 += (unsigned)diff; p = pred2 += (unsigned)diff; }
                    if (WRITE && blk >= 0 && blk < nblk) coef[blk * 64] = (short)(unsigned short)(p & 0xffffu);
                    k = 1;
                }
            }
        } else {
            const int rs = js_symbol(b, huff + 2 + (ta[comp] & 1));
            if (rs == -2) e = JD_ERR_DATA;
            else if (rs == -1) e = b.skip(1) ? JD_ERR_CODE : JD_ERR_DATA;
            else {
                const int r = rs >> 4, s = rs & 15;
                if (s == 0) {
                    if (r != 15) done = true;        // EOB
                    else { k += 16; done = k > 63; }  // ZRL
                } else {
                    k += r;
                    if (k > 63) e = JD_ERR_INDEX;
                    else {
                        const int v = jd_extend((int)b.peek(s), s);
                        if (!b.skip(s)) e = JD_ERR_DATA;
                        else {
                            if (WRITE && blk >= 0 && blk < nblk) coef[blk * 64 + zigzag[k & 63]] = (short)v;
                            done = ++k > 63;
                        }
                    }
                }
            }
        }
        if (e) {
            if (WRITE && blk < nblk) err |= e;
            if (e == JD_ERR_DATA) {                  // nothing is left to decode
                out->pos = end; out->meta = JS_DEAD;
                return err;
            }
            done = true;
        }
        if (done) {
            k = 0;
            j = j + 1 >= bpm ? 0 : j + 1;
        }
    }
}
