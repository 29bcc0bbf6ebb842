// PROB_TO_ID flags == 16384 (ABI 11, form added): the zlib stream of a PNG's IDAT chunk for photographs and smooth planes -- colour types 0, 4,
// 2 and 6 at 8 bits (B = 1 .. 4 bytes per pixel), scanline filters chosen per row, one DEFLATE block per band of PPH_R rows with dynamic
// Huffman codes, or the fixed ones where those are no longer.  (png.hip, flags&8, stays what it is: filter 0 and one fixed block, which suits
// id planes.)  The rule is stated operation by operation in include/cutie_hip.h; tests/png_photo_ref.py is the same rule in numpy; the bytes
// are equal.  ResultSaver(cutout=True, png_codes='dynamic'), cutie_amd/inference/utils/png.py, DESIGN.md section 24.
//
// Five launches (grid-wide dependencies lie between them: a row's tokens need the filtered row above, a band's codes need the counts of
// all its rows, a row's bit offset needs the bit counts of all rows above it):
//   A  pph_filter_kernel  one wave per row: the channels are interleaved from the sources on the fly (no RGBA buffer exists), the five
//                         residuals of every byte depend on raw bytes only and are lane-parallel; the five costs are reduced across the
//                         wave, the chosen filtered row goes to the scratch [H, L], the Adler-32 partials are summed meanwhile.
//   B  pph_token_kernel   one wave per row: equality masks for the distances 1, B and L by ballot into LDS; every lane takes the capped run
//                         lengths at its byte by ctz over the masks.  Token starts: a chunk of 64 bytes is resolved with bit operations on
//                         wave-uniform values -- literal stretches are taken whole, only a MATCH (>= PPH_MINMATCH bytes) costs a step; no
//                         lane walks bytes.  A 16-bit record per byte goes to the scratch; the band's counts are collected in LDS and added
//                         to the band's table with integer vector atomics (sums commute: the bytes do not depend on arrival order).
//   C  pph_codes_kernel   one block per band: rank sort of the symbols (parallel), the two-queue Huffman merge, the length limit and the
//                         code-length code (one lane: <= 286 + 19 symbols, not bytes), canonical codes (parallel), the header bits, the choice
//                         between the fixed and the dynamic form, then the bit count of every row of the band under the chosen codes.
//   D  pph_scan_kernel    one block: exclusive scan of the rows' bit counts, Adler-32 from the partials, length check, status; clears
//                         exactly the words the stream will use and writes the zlib header and the trailer.
//   E  pph_emit_kernel    one wave per row: every lane encodes the token that starts at its byte, a wave prefix sum of the bit lengths
//                         places it, the codes are OR-ed into the row's LDS image (behind the band's header in a band's first row, before
//                         the end-of-block code in its last), and the image is shifted to the row's offset: interior words have one owner,
//                         the shared first and last words are OR-ed in with a vector atomic, as png_emit_kernel does.
// LDS does not lower the row limit: the emit kernel's image of a row at L = 16384 is 32 KB.
#include "common.h"
#include "deflate_enc.h"       // bit writer, symbols, code builder and dynamic header (deflate_enc_core.h), run lengths, scan body, shift-out

#define PPH_MINMATCH 12        // tests/png_photo_ref.py MINMATCH; the table that chose it: DESIGN.md section 24
#define PPH_R 32               // rows per DEFLATE block
#define PPH_RUNCAP 261         // run lengths are counted this far: take() needs no more
#define PPH_ROW_LIMIT CUTIE_PNG_PHOTO_ROW_LIMIT    // L = W B + 1: every distance inside DEFLATE's window
#define PPH_BAND_WORDS 1024    // per band: counts [320] (literal/length 0 .. 285, distance at 288), table [320] (code | bits << 16), info, header
#define PPH_TAB 320
#define PPH_INFO 640           // +0 header bits, +1 form (1 fixed, 2 dynamic), +2 bits of the block
#define PPH_HDR 648
#define PPH_HDR_WORDS (PPH_BAND_WORDS - PPH_HDR)     // 376 words; a header is at most 17 + 57 + 316 * 14 = 4498 bits
#define PPH_DIST 288

struct PphSrc {                // p2 = first source u8 [H, W, c0] with row stride ld0 bytes; p6 = optional plane u8 [H, W], row stride ld1
    const uint8_t* s0;
    const uint8_t* s1;
    int c0, B, ld0, ld1;
};

static inline long pph_up4(long v) { return (v + 3) & ~3l; }
struct PphLayout { long info, band, filt, tok, total; };       // word offsets into the scratch; every one a multiple of 4
static PphLayout pph_layout(long H, long L) {
    PphLayout o;
    const long nb = (H + PPH_R - 1) / PPH_R;
    o.info = 0;
    o.band = 4 * H;
    o.filt = o.band + PPH_BAND_WORDS * nb;
    o.tok = o.filt + pph_up4((H * L + 3) / 4);
    o.total = o.tok + pph_up4((H * L + 1) / 2);
    return o;
}

static_assert(PPH_HDR_WORDS >= DE_HDR_WORDS, "the band's header slot holds any dynamic header");

__device__ __forceinline__ int pph_abs8(uint32_t v) { const int s = (int)(int8_t)(uint8_t)v; return s < 0 ? -s : s; }

// the five residuals of raw byte j of row r (mod 256)
__device__ __forceinline__ void pph_residuals(const PphSrc& S, int r, int j, uint32_t res[5]) {
    const int px = j / S.B, ch = j - px * S.B;
    const uint8_t* q = ch < S.c0 ? S.s0 + (long)r * S.ld0 + (long)px * S.c0 + ch : S.s1 + (long)r * S.ld1 + px;
    const int step = ch < S.c0 ? S.c0 : 1;
    const long ld = ch < S.c0 ? S.ld0 : S.ld1;
    const int x = q[0], a = px > 0 ? q[-step] : 0, b = r > 0 ? q[-ld] : 0, c = (px > 0 && r > 0) ? q[-ld - step] : 0;
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    const int pr = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    res[0] = (uint32_t)x & 255u;
    res[1] = (uint32_t)(x - a) & 255u;
    res[2] = (uint32_t)(x - b) & 255u;
    res[3] = (uint32_t)(x - ((a + b) >> 1)) & 255u;
    res[4] = (uint32_t)(x - pr) & 255u;
}

// A: grid = H rows, block = one wave.  info[r] = {-, sum of the filtered bytes mod 65521, sum of (L - j) * byte_j mod 65521, -}
extern "C" __global__ __launch_bounds__(64) void pph_filter_kernel(PphSrc S, int H, int W, int4* __restrict__ info, uint32_t* __restrict__ band,
                                                                    uint8_t* __restrict__ filt) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int n = W * S.B, L = n + 1;
    if (r % PPH_R == 0) {                                        // the band's counts start at zero (the token kernel adds to them)
        uint32_t* cnt = band + (long)(r / PPH_R) * PPH_BAND_WORDS;
        for (int k = lane; k < PPH_TAB; k += 64) cnt[k] = 0u;
    }
    uint32_t cost[5] = {0u, 0u, 0u, 0u, 0u};
    uint32_t res[5];
    for (int j = lane; j < n; j += 64) {
        pph_residuals(S, r, j, res);
#pragma unroll
        for (int k = 0; k < 5; ++k) cost[k] += (uint32_t)pph_abs8(res[k]);
    }
#pragma unroll
    for (int k = 0; k < 5; ++k)
        for (int o = 32; o > 0; o >>= 1) cost[k] += __shfl_xor(cost[k], o, 64);
    int pick = 0;
#pragma unroll
    for (int k = 1; k < 5; ++k)
        if (cost[k] < cost[pick]) pick = k;                      // strictly lower: ties stay with the lower number
    uint8_t* out = filt + (long)r * L;
    uint64_t Ssum = 0, T = 0;
    if (lane == 0) {
        out[0] = (uint8_t)pick;
        Ssum = (uint64_t)pick;
        T = (uint64_t)L * pick;
    }
    for (int j = lane; j < n; j += 64) {
        pph_residuals(S, r, j, res);
        const uint32_t v = pick == 0 ? res[0] : pick == 1 ? res[1] : pick == 2 ? res[2] : pick == 3 ? res[3] : res[4];
        out[1 + j] = (uint8_t)v;
        Ssum += v;
        T += (uint64_t)(L - 1 - j) * v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        Ssum += __shfl_xor((unsigned long long)Ssum, o, 64);
        T += __shfl_xor((unsigned long long)T, o, 64);
    }
    if (lane == 0) info[r] = make_int4(0, (int)(Ssum % DE_ADLER), (int)(T % DE_ADLER), 0);
}

// B: grid = H rows, block = one wave.  tok[r][i]: 0 = no token starts here | 0x8000 literal | 0x8000 | kind << 9 | length (kind 0: distance
// 1, 1: distance B, 2: distance L)
extern "C" __global__ __launch_bounds__(64) void pph_token_kernel(int H, int L, int B, const uint8_t* __restrict__ filt, uint16_t* __restrict__ tok,
                                                                   uint32_t* __restrict__ band, int dsym1, int dsymB, int dsymL) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int r = blockIdx.x, lane = threadIdx.x;
    const int nmask = (L + 63) >> 6;
    uint64_t* m1 = (uint64_t*)lds;
    uint64_t* mB = m1 + nmask + 1;
    uint64_t* mL = mB + nmask + 1;
    uint32_t* cnt = (uint32_t*)(mL + nmask + 1);
    const uint8_t* row = filt + (long)r * L;
    for (int k = lane; k < PPH_TAB; k += 64) cnt[k] = 0u;
    for (int base = 0; base < nmask * 64; base += 64) {
        const int i = base + lane;
        const bool in = i < L;
        const uint32_t c = in ? row[i] : 0u;
        const uint32_t left = (in && i >= 1) ? row[i - 1] : 0u;
        const uint32_t back = (in && B > 1 && i >= B) ? row[i - B] : 0u;
        const uint32_t up = (in && r > 0) ? row[i - (long)L] : 0u;
        const uint64_t b1 = __ballot(in && i >= 1 && c == left), bB = __ballot(in && B > 1 && i >= B && c == back),
                       bL = __ballot(in && r > 0 && c == up);
        if (lane == 0) { m1[base >> 6] = b1; mB[base >> 6] = bB; mL[base >> 6] = bL; }
    }
    if (lane == 0) m1[nmask] = mB[nmask] = mL[nmask] = 0;
    __syncthreads();
    uint16_t* trow = tok + (long)r * L;
    int entry = 0;                                               // wave-uniform: where the next token starts
    for (int base = 0; base < L; base += 64) {
        const int i = base + lane;
        const bool in = i < L;
        int n = 0, kind = 0;
        if (in) {
            const int n1 = de_run<PPH_RUNCAP>(m1, i, nmask), nB = de_run<PPH_RUNCAP>(mB, i, nmask), nL = de_run<PPH_RUNCAP>(mL, i, nmask);
            n = max(n1, max(nB, nL));
            kind = (n1 >= nB && n1 >= nL) ? 0 : (nB >= nL ? 1 : 2);
        }
        const bool match = in && n >= PPH_MINMATCH;
        const int step = match ? de_take(n) : 1;
        const uint64_t M = __ballot(match);
        uint64_t starts = 0;
        int cur = entry - base;                                  // >= 0
        while (cur < 64) {                                       // one round per match of the chunk, not per byte
            const uint64_t from = ~0ull << cur;
            const uint64_t m = M & from;
            if (m == 0) { starts |= from; cur = 64; break; }
            const int q = __builtin_ctzll(m);
            starts |= from & (q == 63 ? ~0ull : ((1ull << (q + 1)) - 1ull));
            cur = q + __shfl(step, q, 64);
        }
        entry = base + cur;
        const bool start = in && ((starts >> lane) & 1ull);
        uint32_t rec = 0u;
        if (start) {
            rec = 0x8000u;
            if (match) {
                rec |= (uint32_t)kind << 9 | (uint32_t)step;
                int sym, eb;
                uint32_t extra;
                de_len_sym(step, sym, eb, extra);
                atomicAdd(&cnt[sym], 1u);
                atomicAdd(&cnt[PPH_DIST + (kind == 0 ? dsym1 : kind == 1 ? dsymB : dsymL)], 1u);
            } else
                atomicAdd(&cnt[row[i]], 1u);
        }
        if (in) trow[i] = (uint16_t)rec;
    }
    __syncthreads();
    uint32_t* g = band + (long)(r / PPH_R) * PPH_BAND_WORDS;
    for (int k = lane; k < PPH_TAB; k += 64)
        if (cnt[k]) atomicAdd(&g[k], cnt[k]);
}

// bits of the token whose record is `rec` at a byte of value `byte`, under the table `tab`
__device__ __forceinline__ int pph_token_bits(const uint32_t* tab, uint32_t rec, uint32_t byte, int dsym0, int dsym1, int dsym2) {
    if (!(rec & 0x8000u)) return 0;
    const int len = rec & 511u;
    if (len == 0) return (int)(tab[byte] >> 16);
    const int kind = (rec >> 9) & 3u;
    int sym, eb;
    uint32_t extra;
    de_len_sym(len, sym, eb, extra);
    const int ds = kind == 0 ? dsym0 : kind == 1 ? dsym1 : dsym2;
    return (int)(tab[sym] >> 16) + eb + (int)(tab[PPH_DIST + ds] >> 16) + de_d_extra(ds);
}

// C: grid = bands, block = 256
extern "C" __global__ __launch_bounds__(256) void pph_codes_kernel(int H, int L, int4* __restrict__ info, uint32_t* __restrict__ band,
                                                                    const uint8_t* __restrict__ filt, const uint16_t* __restrict__ tok,
                                                                    int dsym1, int dsymB, int dsymL) {
    __shared__ int cnt[PPH_TAB], len[PPH_TAB], A[DE_NSORT], order[DE_NSORT], num[16], dnum[16], clnum[16];
    __shared__ int clcnt[19], cllen[19], clcode[19], nextc[16], dnext[16];
    __shared__ uint32_t tab[PPH_TAB];
    __shared__ uint16_t rle[DE_NRLE];
    __shared__ int n_s, sums[2], rowbits[PPH_R], form_s, hdrbits_s;
    __shared__ uint32_t hdr[PPH_HDR_WORDS];
    const int b = blockIdx.x, t = threadIdx.x;
    const int r0 = b * PPH_R, r1 = min(r0 + PPH_R, H);
    uint32_t* g = band + (long)b * PPH_BAND_WORDS;
    for (int k = t; k < PPH_TAB; k += 256) { cnt[k] = (int)g[k]; len[k] = 0; }
    for (int k = t; k < PPH_HDR_WORDS; k += 256) hdr[k] = 0u;
    if (t < PPH_R) rowbits[t] = 0;
    if (t == 0) { sums[0] = sums[1] = 0; n_s = 0; }
    __syncthreads();
    if (t == 0) cnt[256] += 1;                                   // end-of-block, once
    __syncthreads();
    // rank sort of the literal/length symbols with a count, by (count, symbol)
    for (int s = t; s < 286; s += 256) {
        const int c = cnt[s];
        if (c <= 0) continue;
        int rank = 0;
        for (int u = 0; u < 286; ++u) {
            const int cu = cnt[u];
            rank += (cu > 0 && (cu < c || (cu == c && u < s))) ? 1 : 0;
        }
        A[rank] = c;
        order[rank] = s;
        atomicAdd(&n_s, 1);
    }
    __syncthreads();
    if (t == 0) {
        de_lengths(A, order, n_s, 15, len, num);
        const int nd = de_sort_small(cnt + PPH_DIST, 30, A, order);
        de_lengths(A, order, nd, 15, len + PPH_DIST, dnum);
        de_first_codes(num, 15, nextc);
        de_first_codes(dnum, 15, dnext);
    }
    __syncthreads();
    // canonical codes: the first code of the length plus the symbols of that length in front
    for (int s = t; s < PPH_TAB; s += 256) {
        const bool dist = s >= PPH_DIST;
        const int l = (s < 286 || (dist && s < PPH_DIST + 30)) ? len[s] : 0;
        uint32_t e = 0u;
        if (l) {
            int before = 0;
            for (int u = dist ? PPH_DIST : 0; u < s; ++u) before += len[u] == l ? 1 : 0;
            e = de_rev((uint32_t)((dist ? dnext[l] : nextc[l]) + before), l) | (uint32_t)l << 16;
        }
        tab[s] = e;
        // the two forms' bits of the block's tokens
        const int c = cnt[s];
        if (c > 0 && (s < 286 || dist)) {
            const int ext = dist ? de_d_extra(s - PPH_DIST) : de_ll_extra(s);
            const int fl = dist ? 5 : (int)(de_fixed_ll(s) >> 16);
            atomicAdd(&sums[0], c * (l + ext));
            atomicAdd(&sums[1], c * (fl + ext));
        }
    }
    __syncthreads();
    if (t == 0) {
        const uint32_t final = r1 == H ? 1u : 0u;
        const int hbits = de_dynamic_header(len, len + PPH_DIST, final, A, order, clcnt, cllen, clcode, clnum, rle, hdr).bits;
        const int dyn = hbits + sums[0], fix = 3 + sums[1];
        const bool fixed = fix <= dyn;
        form_s = 2 - (int)((uint32_t)~(dyn - fix) >> 31);          // 1 fixed, 2 dynamic; arithmetic on the sign of dyn - fix (both far below 2^31)
        hdrbits_s = fixed ? 3 : hbits;
        if (fixed) hdr[0] = final | 1u << 1;
        g[PPH_INFO + 0] = (uint32_t)hdrbits_s;
        g[PPH_INFO + 1] = (uint32_t)form_s;
        g[PPH_INFO + 2] = (uint32_t)(fixed ? fix : dyn);
    }
    __syncthreads();
    if (form_s == 1)
        for (int s = t; s < PPH_TAB; s += 256)
            tab[s] = s < 286 ? de_fixed_ll(s) : (s >= PPH_DIST && s < PPH_DIST + 30) ? (de_rev((uint32_t)(s - PPH_DIST), 5) | 5u << 16) : 0u;
    __syncthreads();
    for (int k = t; k < PPH_TAB; k += 256) g[PPH_TAB + k] = tab[k];
    const int hw = (hdrbits_s + 31) >> 5;
    for (int k = t; k < hw; k += 256) g[PPH_HDR + k] = hdr[k];
    // the rows' bit counts under the chosen codes
    for (int r = r0; r < r1; ++r) {
        int bits = 0;
        const uint16_t* trow = tok + (long)r * L;
        const uint8_t* frow = filt + (long)r * L;
        for (int i = t; i < L; i += 256) bits += pph_token_bits(tab, trow[i], frow[i], dsym1, dsymB, dsymL);
        for (int o = 32; o > 0; o >>= 1) bits += __shfl_xor(bits, o, 64);
        if ((t & 63) == 0 && bits) atomicAdd(&rowbits[r - r0], bits);
    }
    __syncthreads();
    if (t < r1 - r0) {
        int bits = rowbits[t];
        if (t == 0) bits += hdrbits_s;
        if (t == r1 - r0 - 1) bits += (int)(tab[256] >> 16);
        info[r0 + t].x = bits;
    }
}

// D: one block (de_scan): 2 header bytes and the blocks -- their headers and end-of-block codes are counted in the rows' bits.  Word 0: the
// zlib header (32K window, no dictionary)
extern "C" __global__ __launch_bounds__(1024) void pph_scan_kernel(int4* __restrict__ info, int H, int L, uint8_t* __restrict__ out, int cap,
                                                                    int* __restrict__ status) {
    de_scan(info, H, L, 16u, 0u, 0x78u | (0x01u << 8), out, cap, status);
}

// E: grid = H rows, block = one wave.  LDS: the band's table, then the row's image
extern "C" __global__ __launch_bounds__(64) void pph_emit_kernel(const int4* __restrict__ info, int H, int L, const uint32_t* __restrict__ band,
                                                                  const uint8_t* __restrict__ filt, const uint16_t* __restrict__ tok,
                                                                  uint32_t* __restrict__ out, const int* __restrict__ status, int imgwords,
                                                                  int dsym1, int dsymB, int dsymL, uint32_t dex1, uint32_t dexB, uint32_t dexL) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    if (status[2] != 0) return;
    const int r = blockIdx.x, lane = threadIdx.x;
    uint32_t* tab = (uint32_t*)lds;
    uint32_t* img = tab + PPH_TAB;
    const int4 v = info[r];
    const uint32_t nbits = (uint32_t)v.x, off = 16u + (uint32_t)v.w;
    const uint32_t* g = band + (long)(r / PPH_R) * PPH_BAND_WORDS;
    const bool first = r % PPH_R == 0, last = r % PPH_R == PPH_R - 1 || r == H - 1;
    const uint32_t nsrc = (nbits + 31) >> 5;
    if ((int)nsrc + 2 > imgwords) return;                         // (cannot happen: the launcher sized the image for any row)
    for (int k = lane; k < PPH_TAB; k += 64) tab[k] = g[PPH_TAB + k];
    for (uint32_t k = lane; k < nsrc + 2; k += 64) img[k] = 0u;
    __syncthreads();
    uint32_t pos = 0;
    if (first) {
        pos = g[PPH_INFO];
        for (uint32_t k = lane; k < (pos + 31) >> 5; k += 64) img[k] = g[PPH_HDR + k];
        __syncthreads();
    }
    const uint16_t* trow = tok + (long)r * L;
    const uint8_t* frow = filt + (long)r * L;
    for (int base = 0; base < L; base += 64) {
        const int i = base + lane;
        const uint32_t rec = i < L ? trow[i] : 0u;
        uint64_t val = 0;
        int nb = 0;
        if (rec & 0x8000u) {
            const int len = rec & 511u;
            if (len == 0) {
                const uint32_t e = tab[frow[i]];
                val = e & 0xffffu;
                nb = (int)(e >> 16);
            } else {
                const int kind = (rec >> 9) & 3u;
                int sym, eb;
                uint32_t extra;
                de_len_sym(len, sym, eb, extra);
                const uint32_t e1 = tab[sym];
                val = e1 & 0xffffu;
                nb = (int)(e1 >> 16);
                val |= (uint64_t)extra << nb;
                nb += eb;
                const int ds = kind == 0 ? dsym1 : kind == 1 ? dsymB : dsymL;
                const uint32_t e2 = tab[PPH_DIST + ds];
                val |= (uint64_t)(e2 & 0xffffu) << nb;
                nb += (int)(e2 >> 16);
                val |= (uint64_t)(kind == 0 ? dex1 : kind == 1 ? dexB : dexL) << nb;
                nb += de_d_extra(ds);                            // <= 15 + 5 + 15 + 13 = 48 bits
            }
        }
        int incl = nb;
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (nb) {
            const uint32_t at = pos + (uint32_t)(incl - nb), w = at >> 5, sh = at & 31u;
            const uint64_t lo = val << sh;
            atomicOr(&img[w], (uint32_t)lo);
            if ((uint32_t)(lo >> 32)) atomicOr(&img[w + 1], (uint32_t)(lo >> 32));
            if (sh && (val >> (64 - sh))) atomicOr(&img[w + 2], (uint32_t)(val >> (64 - sh)));
        }
        pos += (uint32_t)__shfl(incl, 63, 64);
    }
    if (last && lane == 0) {
        const uint32_t e = tab[256], w = pos >> 5, sh = pos & 31u;
        const uint64_t lo = (uint64_t)(e & 0xffffu) << sh;
        atomicOr(&img[w], (uint32_t)lo);
        if ((uint32_t)(lo >> 32)) atomicOr(&img[w + 1], (uint32_t)(lo >> 32));
    }
    __syncthreads();
    if (nbits == 0) return;
    de_shift_out(img, nsrc, nbits, off, out, lane);
}

// PROB_TO_ID flags == 16384 (slots: include/cutie_hip.h).  p2 = first source u8 ([H, W] or [H, W, 3], i3 = its channels, i4 = its row stride
// in bytes), p6 = optional last-channel plane u8 [H, W] (i5 = its row stride), p3 = stream, i7 = capacity, p4 = status int32 [4], p5 = scratch
// int32 [i8]
int launch_png_photo(const cutie_op* op, hipStream_t s) {
    const uint64_t* p = op->p;
    const int* i = op->i;
    const int H = i[1], W = i[2], c0 = i[3], ld0 = i[4], ld1 = i[5];
    const int cap = i[7] & ~3;
    if (H < 1 || W < 1) { cutie_set_error("png photo: H >= 1 and W >= 1, not %d x %d", H, W); return -2; }
    if (c0 != 1 && c0 != 3) { cutie_set_error("png photo: the first source has 1 or 3 channels (i3), not %d", c0); return -2; }
    const int B = c0 + (p[6] ? 1 : 0);
    if ((long)W * B + 1 > PPH_ROW_LIMIT) { cutie_set_error("png photo: a row of %d pixels of %d bytes: W * B + 1 <= %d (every distance inside DEFLATE's window)", W, B, PPH_ROW_LIMIT); return -2; }
    const long L = (long)W * B + 1;
    if (ld0 < W * c0 || (p[6] && ld1 < W)) { cutie_set_error("png photo: row strides (i4 = %d, i5 = %d) below a row's bytes", ld0, ld1); return -2; }
    const long nb = ((long)H + PPH_R - 1) / PPH_R;
    if (9 * L * H + 10 * nb + 64 >= (1l << 31)) { cutie_set_error("png photo: %d x %d x %d exceeds 2^31 stream bits", H, W, B); return -2; }
    if (i[7] < 0) { cutie_set_error("png photo: negative capacity"); return -2; }
    // (a capacity below 4 bytes holds no stream: the overflow bit is set and p3, which may then be null, is never touched)
    if (!p[2] || (!p[3] && cap > 0) || !p[4] || !p[5]) { cutie_set_error("png photo: needs the source (p2), the stream (p3), the status (p4) and the scratch (p5)"); return -2; }
    if ((p[3] & 3) || (p[4] & 3) || (p[5] & 15)) { cutie_set_error("png photo: stream and status 4-byte aligned, scratch 16-byte aligned"); return -2; }
    const PphLayout lay = pph_layout(H, L);
    if ((long)i[8] < lay.total) { cutie_set_error("png photo: scratch of %d words, needs %ld", i[8], lay.total); return -2; }
    uint32_t* base = (uint32_t*)p[5];
    int4* info = (int4*)(base + lay.info);
    uint32_t* band = base + lay.band;
    uint8_t* filt = (uint8_t*)(base + lay.filt);
    uint16_t* tok = (uint16_t*)(base + lay.tok);
    PphSrc S{(const uint8_t*)p[2], (const uint8_t*)p[6], c0, B, ld0, ld1};
    int ds[3], deb[3];
    uint32_t dex[3];
    de_dist_sym(1, ds[0], deb[0], dex[0]);
    de_dist_sym(B, ds[1], deb[1], dex[1]);
    de_dist_sym((int)L, ds[2], deb[2], dex[2]);
    const int nmask = (int)((L + 63) >> 6);
    const size_t lds_tok = (size_t)(3 * (nmask + 1)) * 8 + PPH_TAB * 4;
    const int imgwords = (int)((15 * L + 15 + 31) / 32) + PPH_HDR_WORDS + 4;     // a token costs at most 15 bits per byte it covers
    const size_t lds_emit = (size_t)(PPH_TAB + imgwords) * 4;
    hipLaunchKernelGGL(pph_filter_kernel, dim3(H), dim3(64), 0, s, S, H, W, info, band, filt);
    hipLaunchKernelGGL(pph_token_kernel, dim3(H), dim3(64), lds_tok, s, H, (int)L, B, (const uint8_t*)filt, tok, band, ds[0], ds[1], ds[2]);
    hipLaunchKernelGGL(pph_codes_kernel, dim3((int)nb), dim3(256), 0, s, H, (int)L, info, band, (const uint8_t*)filt, (const uint16_t*)tok, ds[0], ds[1], ds[2]);
    hipLaunchKernelGGL(pph_scan_kernel, dim3(1), dim3(1024), 0, s, info, H, (int)L, (uint8_t*)p[3], cap, (int*)p[4]);
    hipLaunchKernelGGL(pph_emit_kernel, dim3(H), dim3(64), lds_emit, s, (const int4*)info, H, (int)L, (const uint32_t*)band, (const uint8_t*)filt,
                       (const uint16_t*)tok, (uint32_t*)p[3], (const int*)p[4], imgwords, ds[0], ds[1], ds[2], dex[0], dex[1], dex[2]);
    return (int)hipGetLastError();
}
