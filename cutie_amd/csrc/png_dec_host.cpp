// Host check program of the PNG decode (png_dec.hip): the serial core of the kernel, png_inflate_core.h, compiled as plain C++ and run over
// a corpus of packets -- good and corrupt -- on the CPU.  Built with -fsanitize=address,undefined (make -C cutie_amd/csrc png_dec_host, or
// tests/test_png_decode_cpu.py), every buffer is allocated at exactly the size the kernel is told, so a read or write the core's checks let
// through is a sanitizer report here before it is a fault on a GPU.  Nothing of this is loaded into Python or run on a device.
//
//   png_dec_host CORPUS      CORPUS = records of (uint32 little-endian length, packet bytes)
//   one line per record:     index  error bits  bytes produced  blocks  tokens  Adler-32 of the decoded pixels (0 after an error)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "png_inflate_core.h"

static uint32_t adler32(const uint8_t* p, size_t n) {
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < n; ++i) {
        a = (a + p[i]) % 65521u;
        b = (b + a) % 65521u;
    }
    return b << 16 | a;
}

// the unfilter stage, serial: rows in order, the row above the first is zero
static uint32_t unfilter(const PdGeom& g, const uint8_t* in, uint8_t* out) {
    const int rb = g.rowbytes, bpp = g.channels;
    std::vector<uint8_t> prev(rb, 0), cur(rb);
    for (int y = 0; y < g.H; ++y) {
        const uint8_t* src = in + (size_t)y * (rb + 1);
        const int ft = src[0];
        if (ft > 4) return PD_E_FILTER;
        for (int i = 0; i < rb; ++i) {
            const int a = i >= bpp ? cur[i - bpp] : 0, b = prev[i], c = i >= bpp ? prev[i - bpp] : 0;
            const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : pd_paeth(a, b, c);
            cur[i] = (uint8_t)(src[1 + i] + pred);
        }
        if (g.depth == 8) memcpy(out + (size_t)y * rb, cur.data(), rb);
        else
            for (int x = 0; x < g.W; ++x) {
                const int bit = x * g.depth;
                out[(size_t)y * g.W + x] = (uint8_t)((cur[bit >> 3] >> (8 - g.depth - (bit & 7))) & ((1 << g.depth) - 1));
            }
        prev.swap(cur);
    }
    return 0;
}

static void decode(int index, const uint8_t* packet, size_t len) {
    PdGeom g;
    if (!pd_header(packet, (long)len, &g)) {
        printf("%d %u 0 0 0 0\n", index, (unsigned)PD_E_HEADER);
        return;
    }
    // exact-size heap copies: the stream (malloc aligns it as the packet layout does), the inflate buffer, the pixels
    uint8_t* stream = (uint8_t*)malloc(g.stream ? g.stream : 1);
    uint8_t* infl = (uint8_t*)malloc(g.inflated);
    const size_t npix = (size_t)g.H * g.W * g.channels;
    uint8_t* pix = (uint8_t*)malloc(npix);
    memcpy(stream, packet + PD_HDR_BYTES, g.stream);
    PdState s;
    PdTable lt, dt;
    uint8_t lens[320];
    PdTok tok;
    pd_init(&s, stream, g.stream, g.inflated);
    // the bound the kernel's argument rests on: calls <= 8 * stream bytes + inflated bytes (+ the one that ends the decode)
    const unsigned long long bound = 8ull * g.stream + g.inflated + 1;
    unsigned long long calls = 0;
    int r;
    while ((r = pd_next(&s, &lt, &dt, lens, &tok)) == PD_R_TOKEN) {
        pd_execute(&s, &tok, infl);
        if (++calls > bound) {
            fprintf(stderr, "record %d: more than %llu decode steps\n", index, bound);
            exit(3);
        }
    }
    uint32_t err = s.err, sum = 0;
    if (!err && adler32(infl, g.inflated) != s.adler) err |= PD_E_ADLER;
    if (!err) err |= unfilter(g, infl, pix);
    if (!err) sum = adler32(pix, npix);
    printf("%d %u %u %u %u %u\n", index, err, s.pos, s.blocks, s.tokens, sum);
    free(stream);
    free(infl);
    free(pix);
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s CORPUS\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    int index = 0;
    for (;;) {
        uint8_t lb[4];
        if (fread(lb, 1, 4, f) != 4) break;
        const size_t len = (size_t)lb[0] | (size_t)lb[1] << 8 | (size_t)lb[2] << 16 | (size_t)lb[3] << 24;
        uint8_t* packet = (uint8_t*)malloc(len ? len : 1);
        if (fread(packet, 1, len, f) != len) {
            fprintf(stderr, "record %d is cut short\n", index);
            return 2;
        }
        decode(index++, packet, len);
        free(packet);
    }
    fclose(f);
    return 0;
}
