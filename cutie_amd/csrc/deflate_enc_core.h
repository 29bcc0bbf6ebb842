// The scalar core of the two PNG encoders (png.hip, PROB_TO_ID flags&8; png_photo.hip, flags == 16384): the rules of RFC 1951 that both write
// with -- symbols of lengths and distances, the fixed codes, the LSB-first bit writer -- and the code builder of the dynamic blocks: code
// lengths under a limit, canonical codes, the block header.  Plain C++: the kernels run it on one lane with the work arrays in LDS,
// png_enc_host.cpp runs the same lines on the CPU under -fsanitize=address,undefined with every work array its own heap block
// (tests/test_png_photo_cpu.py), and tests/png_ref.py and tests/png_photo_ref.py are the same rules in Python.
// What needs a wave (ballot masks, the scan, the shift to a bit offset) is in deflate_enc.h.
#ifndef CUTIE_DEFLATE_ENC_CORE_H
#define CUTIE_DEFLATE_ENC_CORE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DE_FN __host__ __device__ inline
#else
#define DE_FN inline
#endif

#define DE_ADLER 65521u
#define DE_NSORT 288           // work arrays A / order of de_lengths and de_sort_small: >= 286 literal/length symbols
#define DE_NRLE 320            // code-length symbols of a header: at most 286 + 30
#define DE_HDR_BITS 4498       // a dynamic header is at most 17 + 19 * 3 + 316 * (7 + 7) bits
#define DE_HDR_WORDS ((DE_HDR_BITS + 31) / 32)

DE_FN int de_log2(uint32_t v) {                                  // floor(log2(v)), v >= 1
#if defined(__HIP_DEVICE_COMPILE__)
    return 31 - __clz((int)v);
#else
    return 31 - __builtin_clz(v);
#endif
}

DE_FN uint32_t de_rev(uint32_t code, int n) {                    // Huffman codes go MSB first: the n low bits of `code` reversed; n = 0: 0
#if defined(__HIP_DEVICE_COMPILE__)
    return n ? __brev(code) >> (32 - n) : 0u;
#else
    uint32_t r = 0;
    for (int k = 0; k < n; ++k) r = r << 1 | ((code >> k) & 1u);
    return r;
#endif
}

// a run of n equal bytes gives a match of take(n): no 1- or 2-byte rest is left behind a match of 258
DE_FN int de_take(int n) { return n <= 258 ? n : (n - 258 < 3 ? n - 3 : 258); }

// length 3 .. 258 -> symbol, extra bits, extra value (RFC 1951 3.2.5)
DE_FN void de_len_sym(int len, int& sym, int& eb, uint32_t& extra) {
    const int l = len - 3;
    eb = 0;
    extra = 0;
    if (len == 258) sym = 285;
    else if (l < 8) sym = 257 + l;
    else {
        eb = de_log2((uint32_t)l) - 2;
        sym = 261 + 4 * eb + ((l >> eb) & 3);
        extra = l & ((1 << eb) - 1);
    }
}

// distance 1 .. 32768 -> symbol, extra bits, extra value
DE_FN void de_dist_sym(int dist, int& sym, int& eb, uint32_t& extra) {
    const int d = dist - 1;
    eb = 0;
    extra = 0;
    if (d < 4) sym = d;
    else {
        eb = de_log2((uint32_t)d) - 1;
        sym = 2 * eb + 2 + ((d >> eb) & 1);
        extra = d & ((1 << eb) - 1);
    }
}

DE_FN int de_ll_extra(int s) { return (s < 265 || s == 285) ? 0 : (s - 261) >> 2; }      // extra bits of a literal/length symbol
DE_FN int de_d_extra(int s) { return s < 4 ? 0 : (s - 2) >> 1; }                         // ... of a distance symbol

// the fixed codes (RFC 1951 3.2.6) as code | bits << 16, the code already reversed: a literal, a length symbol 257 .. 285, any of the two
DE_FN uint32_t de_fixed_lit(uint32_t v) { return v < 144 ? de_rev(0x30 + v, 8) | 8u << 16 : de_rev(0x190 + (v - 144), 9) | 9u << 16; }
DE_FN uint32_t de_fixed_len(int s) { return s < 280 ? de_rev((uint32_t)(s - 256), 7) | 7u << 16 : de_rev((uint32_t)(0xC0 + (s - 280)), 8) | 8u << 16; }
DE_FN uint32_t de_fixed_ll(int s) { return s < 256 ? de_fixed_lit((uint32_t)s) : de_fixed_len(s); }

struct DeBits {                         // LSB-first bit writer into 32-bit words (one lane); every word it reaches is written whole
    uint32_t* out;
    uint64_t acc;
    int nacc, nwords;
    DE_FN void put(uint32_t v, int n) {                              // n <= 32, nacc < 32
        acc |= (uint64_t)v << nacc;
        nacc += n;
        if (nacc >= 32) {
            out[nwords++] = (uint32_t)acc;
            acc >>= 32;
            nacc -= 32;
        }
    }
    DE_FN int finish() {                                             // the rest goes out; -> bits written
        if (nacc > 0) out[nwords] = (uint32_t)acc;
        return nwords * 32 + nacc;
    }
};

// Code lengths of the n symbols order[0 .. n) whose counts A[0 .. n) ascend (ties by symbol): the in-place two-queue Huffman merge, depths
// above `limit` (<= 15) folded into it and the Kraft sum repaired, lengths handed out from the end of the list.  num[0 .. 15]: codes per
// length.  A is used up.  One lane.  (The method of Moffat and Katajainen, "In-place calculation of minimum-redundancy codes", 1995.)
DE_FN void de_lengths(int* A, const int* order, int n, int limit, int* len, int* num) {
    for (int k = 0; k <= 15; ++k) num[k] = 0;
    if (n == 0) return;
    if (n == 1) { len[order[0]] = 1; num[1] = 1; return; }
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; }
        else A[next] = A[leaf++];
        if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; }
        else A[next] += A[leaf++];
    }
    A[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
    int avbl = 1, used = 0, dpth = 0, next = n - 1;
    root = n - 2;
    while (avbl > 0) {
        while (root >= 0 && A[root] == dpth) { ++used; --root; }
        while (avbl > used) { A[next--] = dpth; --avbl; }
        avbl = 2 * used;
        ++dpth;
        used = 0;
    }
    for (int k = 0; k < n; ++k) num[A[k] < limit ? A[k] : limit] += 1;
    uint32_t total = 0;
    for (int k = 1; k <= limit; ++k) total += (uint32_t)num[k] << (limit - k);
    while (total > (1u << limit)) {                                 // (a Huffman code is complete: the sum is never below)
        num[limit] -= 1;
        for (int k = limit - 1; k > 0; --k)
            if (num[k]) { num[k] -= 1; num[k + 1] += 2; break; }
        total -= 1;
    }
    int j = n;
    for (int k = 1; k <= limit; ++k)
        for (int c = num[k]; c > 0; --c) len[order[--j]] = k;
}

// the symbols of cnt[0 .. nsym) with a count, sorted by (count, symbol) ascending, by insertion: for the small alphabets.  One lane.
DE_FN int de_sort_small(const int* cnt, int nsym, int* A, int* order) {
    int n = 0;
    for (int s = 0; s < nsym; ++s) {
        const int c = cnt[s];
        if (c <= 0) continue;
        int k = n;
        while (k > 0 && A[k - 1] > c) { A[k] = A[k - 1]; order[k] = order[k - 1]; --k; }
        A[k] = c;
        order[k] = s;
        ++n;
    }
    return n;
}

// first canonical code of every length (RFC 1951 3.2.2) from num[] of de_lengths: next[0 .. limit]
DE_FN void de_first_codes(const int* num, int limit, int* next) {
    int code = 0;
    next[0] = 0;
    for (int k = 1; k <= limit; ++k) {
        code = (code + num[k - 1]) << 1;
        next[k] = code;
    }
}

struct DeHeader { int bits, hlit, hdist, hclen; };

// The header of a dynamic block from the code lengths lllen[286] and dlen[30]: HLIT, HDIST, HCLEN the smallest legal, the HLIT + HDIST
// lengths as one sequence in code-length symbols (greedy: 18 for >= 11 zeros, 17 for >= 3, 16 for >= 3 repeats of the length before), the
// code-length code limited to 7 bits.  Work arrays of the caller: A[DE_NSORT], order[DE_NSORT], clcnt / cllen / clcode [19], clnum[16],
// rle[DE_NRLE] (symbol | extra value << 5); hdr[DE_HDR_WORDS] takes the bits.  cllen is left holding the code-length code.  One lane.
DE_FN DeHeader de_dynamic_header(const int* lllen, const int* dlen, uint32_t final, int* A, int* order, int* clcnt, int* cllen, int* clcode,
                                 int* clnum, uint16_t* rle, uint32_t* hdr) {
    int hlit = 257, hdist = 1;
    for (int s = 257; s < 286; ++s) if (lllen[s]) hlit = s + 1;
    for (int s = 0; s < 30; ++s) if (dlen[s]) hdist = s + 1;
    const int nseq = hlit + hdist;
    for (int k = 0; k < 19; ++k) { clcnt[k] = 0; cllen[k] = 0; }
    int nrle = 0, i = 0, prev = -1;
    while (i < nseq) {
        const int v = i < hlit ? lllen[i] : dlen[i - hlit];
        int run = 1;
        while (i + run < nseq && run < 138) {
            const int k = i + run;
            if ((k < hlit ? lllen[k] : dlen[k - hlit]) != v) break;
            ++run;
        }
        int tk, sym, extra;
        if (v == 0 && run >= 11) { tk = run; sym = 18; extra = tk - 11; }
        else if (v == 0 && run >= 3) { tk = run; sym = 17; extra = tk - 3; }
        else if (v != 0 && prev == v && run >= 3) { tk = run < 6 ? run : 6; sym = 16; extra = tk - 3; }
        else { tk = 1; sym = v; extra = 0; }
        rle[nrle++] = (uint16_t)(sym | extra << 5);
        clcnt[sym] += 1;
        prev = v;
        i += tk;
    }
    const int ncl = de_sort_small(clcnt, 19, A, order);
    de_lengths(A, order, ncl, 7, cllen, clnum);
    int nx[8];
    de_first_codes(clnum, 7, nx);
    for (int s = 0; s < 19; ++s) { const int l = cllen[s]; clcode[s] = l ? (int)de_rev((uint32_t)nx[l]++, l) : 0; }
    const int ord[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int hclen = 4;
    for (int k = 0; k < 19; ++k) if (cllen[ord[k]] && k + 1 > hclen) hclen = k + 1;
    DeBits w{hdr, 0ull, 0, 0};
    w.put(final | 2u << 1, 3);
    w.put((uint32_t)(hlit - 257), 5);
    w.put((uint32_t)(hdist - 1), 5);
    w.put((uint32_t)(hclen - 4), 4);
    for (int k = 0; k < hclen; ++k) w.put((uint32_t)cllen[ord[k]], 3);
    for (int k = 0; k < nrle; ++k) {
        const int sym = rle[k] & 31, extra = rle[k] >> 5;
        w.put((uint32_t)clcode[sym], cllen[sym]);
        if (sym == 16) w.put((uint32_t)extra, 2);
        else if (sym == 17) w.put((uint32_t)extra, 3);
        else if (sym == 18) w.put((uint32_t)extra, 7);
    }
    return DeHeader{w.finish(), hlit, hdist, hclen};
}

#endif
