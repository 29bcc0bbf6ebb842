// Host check program of the PNG encoders (png.hip, png_photo.hip): their scalar core, deflate_enc_core.h, compiled as plain C++ and run over
// count vectors on the CPU.  Built with -fsanitize=address,undefined (make -C cutie_amd/csrc png_enc_host, or tests/test_png_photo_cpu.py),
// every work array is its own heap block of exactly the size pph_codes_kernel gives it in LDS, so a write past one is a sanitizer report
// here and not a silent write into the neighbour array.  Nothing of this is loaded into Python or run on a device.
//
//   png_enc_host [RECORDS]   RECORDS (or stdin) = whitespace-separated text, one record after the other:
//     H final c[286] d[30]   a block's counts (end-of-block included) -> what pph_codes_kernel derives from them, one line each:
//                              ll <286 lengths> | dd <30 lengths> | llcode <286 codes, reversed> | dcode <30 codes> |
//                              hdr <bits> <bytes in hex> | h <hlit> <hdist> <hclen> | cl <19 lengths of the code-length code>
//     L limit n c[n]         de_lengths alone on n <= 288 counts -> len <n lengths>
//     S                      every symbol function over its whole domain -> lensym (length 3 .. 258: symbol, extra bits, extra value) |
//                              distsym (distance 1 .. 32768: the same) | take (n = 0 .. 600) | llextra (symbol 0 .. 285) | dextra (0 .. 29) |
//                              fixed (symbol 0 .. 285: code, bits) | rev0 (de_rev(x, 0))
#include <stdio.h>
#include <stdlib.h>

#include "deflate_enc_core.h"

template <class T>
static T* block(size_t n) { return (T*)calloc(n ? n : 1, sizeof(T)); }

static FILE* in;

static int next_int() {
    int v;
    if (fscanf(in, "%d", &v) != 1) {
        fprintf(stderr, "a record is cut short\n");
        exit(2);
    }
    return v;
}

static void line(const char* tag, const int* v, int n) {
    printf("%s", tag);
    for (int k = 0; k < n; ++k) printf(" %d", v[k]);
    printf("\n");
}

// canonical codes of len[0 .. n) from the first code per length, as the kernel's tab[] holds them: reversed
static void codes(const int* len, int n, const int* first, int* code) {
    int nx[16];
    for (int k = 0; k < 16; ++k) nx[k] = first[k];
    for (int s = 0; s < n; ++s) code[s] = len[s] ? (int)de_rev((uint32_t)nx[len[s]]++, len[s]) : 0;
}

static void header_record() {
    const uint32_t final = (uint32_t)next_int() & 1u;
    int* cnt = block<int>(286);
    int* dcnt = block<int>(30);
    for (int s = 0; s < 286; ++s) cnt[s] = next_int();
    for (int s = 0; s < 30; ++s) dcnt[s] = next_int();
    int* lllen = block<int>(286);
    int* dlen = block<int>(30);
    int* A = block<int>(DE_NSORT);
    int* order = block<int>(DE_NSORT);
    int* num = block<int>(16);
    int* dnum = block<int>(16);
    int* clnum = block<int>(16);
    int* nextc = block<int>(16);
    int* dnext = block<int>(16);
    int* clcnt = block<int>(19);
    int* cllen = block<int>(19);
    int* clcode = block<int>(19);
    uint16_t* rle = block<uint16_t>(DE_NRLE);
    uint32_t* hdr = block<uint32_t>(DE_HDR_WORDS);
    int* llcode = block<int>(286);
    int* dcode = block<int>(30);
    // (the kernel rank-sorts the 286 counts in parallel; the insertion sort gives the same order: count, then symbol)
    const int n = de_sort_small(cnt, 286, A, order);
    de_lengths(A, order, n, 15, lllen, num);
    const int nd = de_sort_small(dcnt, 30, A, order);
    de_lengths(A, order, nd, 15, dlen, dnum);
    de_first_codes(num, 15, nextc);
    de_first_codes(dnum, 15, dnext);
    codes(lllen, 286, nextc, llcode);
    codes(dlen, 30, dnext, dcode);
    const DeHeader h = de_dynamic_header(lllen, dlen, final, A, order, clcnt, cllen, clcode, clnum, rle, hdr);
    line("ll", lllen, 286);
    line("dd", dlen, 30);
    line("llcode", llcode, 286);
    line("dcode", dcode, 30);
    printf("hdr %d ", h.bits);
    for (int k = 0; k < (h.bits + 7) / 8; ++k) printf("%02x", (unsigned)(hdr[k >> 2] >> (8 * (k & 3))) & 255u);
    printf("\nh %d %d %d\n", h.hlit, h.hdist, h.hclen);
    line("cl", cllen, 19);
    void* all[] = {cnt, dcnt, lllen, dlen, A, order, num, dnum, clnum, nextc, dnext, clcnt, cllen, clcode, rle, hdr, llcode, dcode};
    for (void* p : all) free(p);
}

static void lengths_record() {
    const int limit = next_int(), n = next_int();
    if (limit < 1 || limit > 15 || n < 0 || n > DE_NSORT) {
        fprintf(stderr, "L: limit 1 .. 15 and at most %d counts\n", DE_NSORT);
        exit(2);
    }
    int* cnt = block<int>(n);
    for (int s = 0; s < n; ++s) cnt[s] = next_int();
    int* len = block<int>(n);
    int* A = block<int>(DE_NSORT);
    int* order = block<int>(DE_NSORT);
    int* num = block<int>(16);
    de_lengths(A, order, de_sort_small(cnt, n, A, order), limit, len, num);
    line("len", len, n);
    free(cnt), free(len), free(A), free(order), free(num);
}

static void symbols_record() {
    int sym, eb;
    uint32_t extra;
    printf("lensym");
    for (int l = 3; l <= 258; ++l) { de_len_sym(l, sym, eb, extra); printf(" %d %d %u", sym, eb, extra); }
    printf("\ndistsym");
    for (int d = 1; d <= 32768; ++d) { de_dist_sym(d, sym, eb, extra); printf(" %d %d %u", sym, eb, extra); }
    printf("\ntake");
    for (int n = 0; n <= 600; ++n) printf(" %d", de_take(n));
    printf("\nllextra");
    for (int s = 0; s < 286; ++s) printf(" %d", de_ll_extra(s));
    printf("\ndextra");
    for (int s = 0; s < 30; ++s) printf(" %d", de_d_extra(s));
    printf("\nfixed");
    for (int s = 0; s < 286; ++s) printf(" %u %u", de_fixed_ll(s) & 0xffffu, de_fixed_ll(s) >> 16);
    printf("\nrev0 %u\n", de_rev(0xffffffffu, 0));
}

int main(int argc, char** argv) {
    if (argc > 2) {
        fprintf(stderr, "usage: %s [RECORDS]\n", argv[0]);
        return 2;
    }
    in = argc == 2 ? fopen(argv[1], "r") : stdin;
    if (!in) {
        perror(argv[1]);
        return 2;
    }
    char kind[8];
    while (fscanf(in, "%7s", kind) == 1) {
        if (kind[0] == 'H') header_record();
        else if (kind[0] == 'L') lengths_record();
        else if (kind[0] == 'S') symbols_record();
        else {
            fprintf(stderr, "unknown record '%s'\n", kind);
            return 2;
        }
    }
    if (in != stdin) fclose(in);
    return 0;
}
