// The serial core of the PNG decode stages (png_dec.hip; RESIZE flags 64 / 128, include/cutie_hip.h ABI 11, forms added): packet header check, bit
// reader, canonical Huffman tables (RFC 1951 3.2.2) and the token decoder of a zlib stream (RFC 1950 / 1951).  Plain C++: the kernel
// runs it on one lane with the tables in LDS, png_dec_host.cpp runs the same lines on the CPU under -fsanitize=address,undefined over the
// whole test corpus, corrupt files included, and tests/png_dec_ref.py is the same rule in Python.
//
// The decoder turns the stream into TOKENS -- a literal, a match (length, distance), a stored run (length, offset into the stream) --
// each with the output position it starts at.  Every check happens HERE, at decode time, where the position is known; executing a token
// is a plain copy inside ranges this file has already checked:
//   - a read of the stream is pd_refill's `pos < n` (or `pos + 4 <= n` for the aligned word) and the stored run's `spos + len <= n`;
//   - a token is handed out only if pos + len <= out_len, so every write lies in [0, out_len);
//   - a match is handed out only if 1 <= dist <= pos, so every read lies in [0, pos) -- never before the buffer.
// Bounded work: every call of pd_next either consumes at least one bit of the stream (a block header is 3 bits, a symbol at least 1),
// or hands out a token of at least one output byte, or ends the decode (error or trailer).  So the calls are at most 8 * stream bytes +
// inflated bytes, whatever the bytes are.  The steps per call are bounded too, by a constant that is not small: a symbol is at most 15
// steps; a dynamic block header reads at most 19 + 316 code lengths and builds three tables, about 1300 steps for at least 17 + 3 bits of
// input; the fixed tables (about 1000 steps) are built once for a run of fixed blocks and again only after a dynamic block, which itself
// took at least 20 bits.  The worst stream -- dynamic and fixed headers alternating, no data -- therefore costs below 100 lane steps
// per input bit: linear in the stream, with that constant.
// The first error ends the decode: its bit is kept in `err`, the tokens handed out before it stay valid.
#ifndef CUTIE_PNG_INFLATE_CORE_H
#define CUTIE_PNG_INFLATE_CORE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PD_FN __host__ __device__ inline
#else
#define PD_FN inline
#endif

// error bits of status word 0
#define PD_E_BTYPE 1       // reserved block type 3
#define PD_E_LENGTHS 2     // over-subscribed or incomplete code lengths, a repeat without a previous length or past the table, no end-of-block code
#define PD_E_SYMBOL 4      // a bit pattern that is no code; literal/length symbol 286 / 287, distance symbol 30 / 31
#define PD_E_DIST 8        // distance beyond the bytes produced so far
#define PD_E_EOF 16        // the stream ends early (inside a block or the Adler-32 trailer)
#define PD_E_SIZE 32       // the output would exceed, or falls short of, the inflated length of the header
#define PD_E_STORED 64     // stored block: LEN != ~NLEN
#define PD_E_ADLER 128     // Adler-32 of the output differs from the trailer
#define PD_E_FILTER 256    // a row's filter byte is above 4
#define PD_E_HEADER 512    // the packet header or its table entry is inconsistent, or the zlib header is not deflate / 32K window class

// packet header: 8 little-endian int32 words, then the zlib stream
#define PD_MAGIC 0x44474E50            // 'PNGD'
#define PD_HDR_WORDS 8
#define PD_HDR_BYTES 32
#define PD_MAX_ROWBYTES 16384          // the unfilter stage keeps two rows in LDS
enum { PD_H_MAGIC = 0, PD_H_W, PD_H_H, PD_H_DEPTH, PD_H_CHANNELS, PD_H_ROWBYTES, PD_H_STREAM, PD_H_INFLATED };

struct PdGeom {
    int W, H, depth, channels, rowbytes;
    uint32_t stream, inflated;
};

// The header of a packet of `avail` bytes (what lies between its offset and the end of the packet buffer) -> geometry, or false.
PD_FN bool pd_header(const uint8_t* pkt, long avail, PdGeom* g) {
    if (avail < PD_HDR_BYTES) return false;
    int32_t h[PD_HDR_WORDS];
    for (int k = 0; k < PD_HDR_WORDS; ++k)
        h[k] = (int32_t)((uint32_t)pkt[4 * k] | (uint32_t)pkt[4 * k + 1] << 8 | (uint32_t)pkt[4 * k + 2] << 16 | (uint32_t)pkt[4 * k + 3] << 24);
    if (h[PD_H_MAGIC] != PD_MAGIC) return false;
    g->W = h[PD_H_W]; g->H = h[PD_H_H]; g->depth = h[PD_H_DEPTH]; g->channels = h[PD_H_CHANNELS]; g->rowbytes = h[PD_H_ROWBYTES];
    if (g->W < 1 || g->H < 1) return false;
    if (!(g->depth == 8 || ((g->depth == 1 || g->depth == 2 || g->depth == 4) && g->channels == 1))) return false;
    if (g->channels != 1 && g->channels != 3) return false;
    const long bits = (long)g->W * g->channels * g->depth;
    if ((bits + 7) / 8 != g->rowbytes || g->rowbytes > PD_MAX_ROWBYTES) return false;
    const long infl = (long)g->H * (g->rowbytes + 1);
    if (infl >= (1l << 31) || h[PD_H_INFLATED] != (int32_t)infl) return false;
    if (h[PD_H_STREAM] < 0 || (long)h[PD_H_STREAM] > avail - PD_HDR_BYTES) return false;
    g->stream = (uint32_t)h[PD_H_STREAM];
    g->inflated = (uint32_t)infl;
    return true;
}

struct PdTable {                 // canonical code: count[l] codes of length l, their symbols in code order
    uint16_t count[16];
    uint16_t symbol[288];
};

enum { PD_TOK_LITERAL = 0, PD_TOK_MATCH = 1, PD_TOK_STORED = 2 };
struct PdTok {
    uint32_t kind, pos, len, arg;    // arg: the byte | the distance | the offset of the run in the stream
};

enum { PD_PH_BLOCK = 0, PD_PH_STORED, PD_PH_CODED, PD_PH_DONE };
enum { PD_R_TOKEN = 0, PD_R_DONE = 1, PD_R_ERROR = 2 };

struct PdState {
    const uint8_t* src;          // the zlib stream, 4-byte aligned
    uint32_t n, spos;            // its bytes; the next byte to load
    uint64_t bits;               // LSB first
    int nbits;
    uint32_t out_len, pos;       // inflated length; bytes produced by the tokens handed out
    uint32_t err, blocks, tokens, adler;
    int phase, final_block, fixed_loaded;   // fixed_loaded: lt / dt hold the fixed codes (built once for consecutive fixed blocks)
    uint32_t stored_left;
};

PD_FN void pd_refill(PdState* s) {
    if (s->nbits <= 32 && (s->spos & 3u) == 0 && s->spos + 4 <= s->n) {        // (n < 2^31: no wrap)
        uint32_t w;                                                             // (one aligned 32-bit load: the stream is 4-byte aligned)
        __builtin_memcpy(&w, __builtin_assume_aligned(s->src + s->spos, 4), 4);
        s->bits |= (uint64_t)w << s->nbits;
        s->nbits += 32;
        s->spos += 4;
    }
    while (s->nbits <= 56 && s->spos < s->n) {
        s->bits |= (uint64_t)s->src[s->spos++] << s->nbits;
        s->nbits += 8;
    }
}

// k <= 32 bits, or false with PD_E_EOF
PD_FN bool pd_get(PdState* s, int k, uint32_t* v) {
    if (s->nbits < k) {
        pd_refill(s);
        if (s->nbits < k) { s->err |= PD_E_EOF; return false; }
    }
    *v = (uint32_t)(s->bits & ((1ull << k) - 1));
    s->bits >>= k;
    s->nbits -= k;
    return true;
}

// zlib's rule (inftrees.c): over-subscribed is an error; incomplete is an error unless the code is a single code of length 1 (what
// zlib's deflate writes for one distance) or empty; the code-length code (strict) must be complete.
PD_FN bool pd_build(PdTable* t, const uint8_t* lens, int n, bool strict) {
    for (int l = 0; l < 16; ++l) t->count[l] = 0;
    for (int k = 0; k < n; ++k) t->count[lens[k]]++;
    int left = 1, maxlen = 0;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - (int)t->count[l];
        if (left < 0) return false;
        if (t->count[l]) maxlen = l;
    }
    if (left > 0 && (strict || maxlen > 1)) return false;
    uint16_t offs[16];
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + t->count[l]);
    for (int k = 0; k < n; ++k)
        if (lens[k]) t->symbol[offs[lens[k]]++] = (uint16_t)k;
    return true;
}

// one symbol, bit by bit (codes are packed MSB first): -> the symbol, or -1 with PD_E_SYMBOL / PD_E_EOF
PD_FN int pd_symbol(PdState* s, const PdTable* t) {
    if (s->nbits < 15) pd_refill(s);
    int code = 0, first = 0, index = 0;
    uint64_t b = s->bits;
    const int avail = s->nbits < 15 ? s->nbits : 15;
    for (int l = 1; l <= avail; ++l) {
        code |= (int)(b & 1);
        b >>= 1;
        const int c = t->count[l];
        if (code - c < first) {
            s->bits >>= l;
            s->nbits -= l;
            return t->symbol[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    s->err |= avail < 15 ? PD_E_EOF : PD_E_SYMBOL;
    return -1;
}

PD_FN void pd_init(PdState* s, const uint8_t* stream, uint32_t n, uint32_t out_len) {
    s->src = stream; s->n = n; s->spos = 0; s->bits = 0; s->nbits = 0;
    s->out_len = out_len; s->pos = 0; s->err = 0; s->blocks = 0; s->tokens = 0; s->adler = 0;
    s->phase = PD_PH_BLOCK; s->final_block = 0; s->fixed_loaded = 0; s->stored_left = 0;
    uint32_t cmf, flg;                                   // RFC 1950: deflate, window <= 32K, no preset dictionary, check bits
    if (!pd_get(s, 8, &cmf) || !pd_get(s, 8, &flg)) return;
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || (flg & 32) || ((cmf << 8) | flg) % 31 != 0) s->err |= PD_E_HEADER;
}

// The tables of a dynamic block (RFC 1951 3.2.7).  `lens` = 320 bytes of scratch.
PD_FN bool pd_dynamic(PdState* s, PdTable* lt, PdTable* dt, uint8_t* lens) {
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t v;
    if (!pd_get(s, 14, &v)) return false;
    const int nlen = (int)(v & 31) + 257, ndist = (int)((v >> 5) & 31) + 1, ncode = (int)(v >> 10) + 4;
    if (nlen > 286 || ndist > 30) { s->err |= PD_E_LENGTHS; return false; }
    for (int k = 0; k < 19; ++k) lens[k] = 0;
    for (int k = 0; k < ncode; ++k) {
        if (!pd_get(s, 3, &v)) return false;
        lens[order[k]] = (uint8_t)v;
    }
    if (!pd_build(lt, lens, 19, true)) { s->err |= PD_E_LENGTHS; return false; }     // (lt holds the code-length code meanwhile)
    int k = 0;
    while (k < nlen + ndist) {
        const int sym = pd_symbol(s, lt);
        if (sym < 0) return false;
        if (sym < 16) { lens[k++] = (uint8_t)sym; continue; }
        int rep, val = 0;
        if (sym == 16) {
            if (k == 0) { s->err |= PD_E_LENGTHS; return false; }
            val = lens[k - 1];
            if (!pd_get(s, 2, &v)) return false;
            rep = 3 + (int)v;
        } else if (sym == 17) {
            if (!pd_get(s, 3, &v)) return false;
            rep = 3 + (int)v;
        } else {
            if (!pd_get(s, 7, &v)) return false;
            rep = 11 + (int)v;
        }
        if (k + rep > nlen + ndist) { s->err |= PD_E_LENGTHS; return false; }
        while (rep--) lens[k++] = (uint8_t)val;
    }
    if (lens[256] == 0) { s->err |= PD_E_LENGTHS; return false; }
    if (!pd_build(dt, lens + nlen, ndist, false)) { s->err |= PD_E_LENGTHS; return false; }   // before lt: lens is read, not changed
    if (!pd_build(lt, lens, nlen, false)) { s->err |= PD_E_LENGTHS; return false; }
    return true;
}

PD_FN void pd_fixed(PdTable* lt, PdTable* dt, uint8_t* lens) {
    int k = 0;
    for (; k < 144; ++k) lens[k] = 8;
    for (; k < 256; ++k) lens[k] = 9;
    for (; k < 280; ++k) lens[k] = 7;
    for (; k < 288; ++k) lens[k] = 8;
    pd_build(lt, lens, 288, false);
    for (k = 0; k < 32; ++k) lens[k] = 5;           // 32 codes make the code complete; symbols 30 / 31 are refused where they are decoded
    pd_build(dt, lens, 32, false);
}

// The next token -> PD_R_TOKEN (tok filled), PD_R_DONE (the final block and the trailer are read; s->adler = the trailer) or PD_R_ERROR.
PD_FN int pd_next(PdState* s, PdTable* lt, PdTable* dt, uint8_t* lens, PdTok* tok) {
    const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                8193, 12289, 16385, 24577};
    const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    uint32_t v;
    if (s->err) return PD_R_ERROR;
    for (;;) {
        if (s->phase == PD_PH_DONE) return PD_R_DONE;
        if (s->phase == PD_PH_BLOCK) {
            if (s->final_block) {                        // trailer: the rest of the byte is dropped, then Adler-32, big-endian
                uint32_t a = 0;
                if (!pd_get(s, s->nbits & 7, &v)) return PD_R_ERROR;
                for (int k = 0; k < 4; ++k) {
                    if (!pd_get(s, 8, &v)) return PD_R_ERROR;
                    a = a << 8 | v;
                }
                s->adler = a;
                if (s->pos != s->out_len) { s->err |= PD_E_SIZE; return PD_R_ERROR; }
                s->phase = PD_PH_DONE;
                return PD_R_DONE;
            }
            if (!pd_get(s, 3, &v)) return PD_R_ERROR;
            s->final_block = (int)(v & 1);
            s->blocks++;
            const int type = (int)(v >> 1);
            if (type == 3) { s->err |= PD_E_BTYPE; return PD_R_ERROR; }
            if (type == 0) {
                uint32_t len, nlen;
                if (!pd_get(s, s->nbits & 7, &v) || !pd_get(s, 16, &len) || !pd_get(s, 16, &nlen)) return PD_R_ERROR;
                if ((len ^ nlen) != 0xffffu) { s->err |= PD_E_STORED; return PD_R_ERROR; }
                s->stored_left = len;
                s->phase = PD_PH_STORED;
            } else {
                if (type == 1) {
                    if (!s->fixed_loaded) pd_fixed(lt, dt, lens);
                    s->fixed_loaded = 1;
                } else {
                    s->fixed_loaded = 0;
                    if (!pd_dynamic(s, lt, dt, lens)) return PD_R_ERROR;
                }
                s->phase = PD_PH_CODED;
            }
            continue;
        }
        if (s->phase == PD_PH_STORED) {
            if (s->stored_left == 0) { s->phase = PD_PH_BLOCK; continue; }
            // the run starts at a byte boundary: the bytes waiting in the bit buffer go back to the stream first
            s->spos -= (uint32_t)(s->nbits >> 3);
            s->bits = 0;
            s->nbits = 0;
            const uint32_t len = s->stored_left;
            if (len > s->n - s->spos) { s->err |= PD_E_EOF; return PD_R_ERROR; }
            if (len > s->out_len - s->pos) { s->err |= PD_E_SIZE; return PD_R_ERROR; }
            tok->kind = PD_TOK_STORED; tok->pos = s->pos; tok->len = len; tok->arg = s->spos;
            s->spos += len;
            s->pos += len;
            s->stored_left = 0;
            s->tokens++;
            return PD_R_TOKEN;
        }
        // PD_PH_CODED
        const int sym = pd_symbol(s, lt);
        if (sym < 0) return PD_R_ERROR;
        if (sym < 256) {
            if (s->pos >= s->out_len) { s->err |= PD_E_SIZE; return PD_R_ERROR; }
            tok->kind = PD_TOK_LITERAL; tok->pos = s->pos; tok->len = 1; tok->arg = (uint32_t)sym;
            s->pos += 1;
            s->tokens++;
            return PD_R_TOKEN;
        }
        if (sym == 256) { s->phase = PD_PH_BLOCK; continue; }
        if (sym > 285) { s->err |= PD_E_SYMBOL; return PD_R_ERROR; }
        if (!pd_get(s, lext[sym - 257], &v)) return PD_R_ERROR;
        const uint32_t len = lbase[sym - 257] + v;
        const int ds = pd_symbol(s, dt);
        if (ds < 0) return PD_R_ERROR;
        if (ds > 29) { s->err |= PD_E_SYMBOL; return PD_R_ERROR; }
        if (!pd_get(s, dext[ds], &v)) return PD_R_ERROR;
        const uint32_t dist = dbase[ds] + v;
        if (dist > s->pos) { s->err |= PD_E_DIST; return PD_R_ERROR; }
        if (len > s->out_len - s->pos) { s->err |= PD_E_SIZE; return PD_R_ERROR; }
        tok->kind = PD_TOK_MATCH; tok->pos = s->pos; tok->len = len; tok->arg = dist;
        s->pos += len;
        s->tokens++;
        return PD_R_TOKEN;
    }
}

// Executing a token: plain copies inside ranges pd_next has checked.  The kernel spreads the same copies over the wave.
PD_FN void pd_execute(const PdState* s, const PdTok* t, uint8_t* out) {
    if (t->kind == PD_TOK_LITERAL) out[t->pos] = (uint8_t)t->arg;
    else if (t->kind == PD_TOK_MATCH)
        for (uint32_t k = 0; k < t->len; ++k) out[t->pos + k] = out[t->pos - t->arg + (k % t->arg)];
    else
        for (uint32_t k = 0; k < t->len; ++k) out[t->pos + k] = s->src[t->arg + k];
}

PD_FN int pd_paeth(int a, int b, int c) {
    const int p = a + b - c;
    int pa = p - a, pb = p - b, pc = p - c;
    pa = pa < 0 ? -pa : pa; pb = pb < 0 ? -pb : pb; pc = pc < 0 ? -pc : pc;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

#endif
