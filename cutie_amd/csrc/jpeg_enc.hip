// PROB_TO_ID flags == 128 (ABI 11): the entropy-coded segment of a baseline JPEG -- 4:2:0, the standard Huffman tables, no restart markers --
// of a uint8 frame [H, W, 3], optionally with the object colours blended over it by an id plane: the bytes libjpeg-turbo's encoder
// writes for the blended frame (PIL's Image.save(x.jpg)), so that `eval_vos --visualize --overlay device` writes the host path's files
// (ResultSaver overlay='device', cutie_amd/inference/utils/results_utils.py; container: cutie_amd/inference/utils/jpeg_writer.py).
// The rules -- blend, colour conversion, edge padding, dummy blocks, FDCT, quantisation, coding -- are listed in include/cutie_hip.h;
// tests/jpeg_enc_ref.py is the same in numpy, the bytes are equal.
//
// The stream is ONE bit string, so two grid-wide dependencies lie between the kernels: the bit offset of a block is the sum of the bits of
// all blocks coded before it, and the byte offset of a chunk after stuffing is its offset plus the 0xFF bytes in front of it.
//   A  jpg_transform_kernel   8 threads per coded block: blend -> YCbCr -> (h2v2 downsample) -> ISLOW FDCT -> quantise; int16 zigzag
//                             coefficients per coded block (MCU by MCU: Y00 Y01 Y10 Y11 Cb Cr) into the scratch
//   B  jpg_count_kernel       one wave per block, one lane per coefficient: no lane walks the block -- the zero runs come from a ballot, the
//                             positions from a wave scan of the lanes' code lengths; -> bits per block
//   C  jpg_scan_bits_kernel   one workgroup, fixed order: bit offsets of the blocks, bytes of the unstuffed stream
//   D  jpg_clear_kernel       clears the words the unstuffed stream will use
//   E  jpg_emit_kernel        B's code again, now written: the block's bits are put together in LDS and shifted to their offset; words shared
//                             with a neighbouring block are merged with vector atomics (OR: the order of arrival does not matter)
//   F  jpg_ff_count_kernel    0xFF bytes per 64-byte chunk of the unstuffed stream
//   G  jpg_scan_ff_kernel     one workgroup, fixed order: the chunks' offsets after stuffing, capacity check, status block
//   H  jpg_write_kernel       the stuffed bytes
// Every offset comes from a scan in a fixed order and every merge is an OR: the bytes depend on the inputs alone.
#include "common.h"

static __device__ const unsigned char JPG_ZZ_OF_NATURAL[64] = {
    0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42,
    3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
    21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63,
};
static __device__ const uint32_t JPG_DC[2][12] = {{
    0x020000, 0x030002, 0x030003, 0x030004, 0x030005, 0x030006, 0x04000e, 0x05001e, 0x06003e, 0x07007e, 0x0800fe, 0x0901fe,
}, {
    0x020000, 0x020001, 0x020002, 0x030006, 0x04000e, 0x05001e, 0x06003e, 0x07007e, 0x0800fe, 0x0901fe, 0x0a03fe, 0x0b07fe,
}};
static __device__ const uint32_t JPG_AC[2][256] = {{
    0x04000a, 0x020000, 0x020001, 0x030004, 0x04000b, 0x05001a, 0x070078, 0x0800f8, 0x0a03f6, 0x10ff82, 0x10ff83, 0, 0, 0, 0, 0,
    0, 0x04000c, 0x05001b, 0x070079, 0x0901f6, 0x0b07f6, 0x10ff84, 0x10ff85, 0x10ff86, 0x10ff87, 0x10ff88, 0, 0, 0, 0, 0,
    0, 0x05001c, 0x0800f9, 0x0a03f7, 0x0c0ff4, 0x10ff89, 0x10ff8a, 0x10ff8b, 0x10ff8c, 0x10ff8d, 0x10ff8e, 0, 0, 0, 0, 0,
    0, 0x06003a, 0x0901f7, 0x0c0ff5, 0x10ff8f, 0x10ff90, 0x10ff91, 0x10ff92, 0x10ff93, 0x10ff94, 0x10ff95, 0, 0, 0, 0, 0,
    0, 0x06003b, 0x0a03f8, 0x10ff96, 0x10ff97, 0x10ff98, 0x10ff99, 0x10ff9a, 0x10ff9b, 0x10ff9c, 0x10ff9d, 0, 0, 0, 0, 0,
    0, 0x07007a, 0x0b07f7, 0x10ff9e, 0x10ff9f, 0x10ffa0, 0x10ffa1, 0x10ffa2, 0x10ffa3, 0x10ffa4, 0x10ffa5, 0, 0, 0, 0, 0,
    0, 0x07007b, 0x0c0ff6, 0x10ffa6, 0x10ffa7, 0x10ffa8, 0x10ffa9, 0x10ffaa, 0x10ffab, 0x10ffac, 0x10ffad, 0, 0, 0, 0, 0,
    0, 0x0800fa, 0x0c0ff7, 0x10ffae, 0x10ffaf, 0x10ffb0, 0x10ffb1, 0x10ffb2, 0x10ffb3, 0x10ffb4, 0x10ffb5, 0, 0, 0, 0, 0,
    0, 0x0901f8, 0x0f7fc0, 0x10ffb6, 0x10ffb7, 0x10ffb8, 0x10ffb9, 0x10ffba, 0x10ffbb, 0x10ffbc, 0x10ffbd, 0, 0, 0, 0, 0,
    0, 0x0901f9, 0x10ffbe, 0x10ffbf, 0x10ffc0, 0x10ffc1, 0x10ffc2, 0x10ffc3, 0x10ffc4, 0x10ffc5, 0x10ffc6, 0, 0, 0, 0, 0,
    0, 0x0901fa, 0x10ffc7, 0x10ffc8, 0x10ffc9, 0x10ffca, 0x10ffcb, 0x10ffcc, 0x10ffcd, 0x10ffce, 0x10ffcf, 0, 0, 0, 0, 0,
    0, 0x0a03f9, 0x10ffd0, 0x10ffd1, 0x10ffd2, 0x10ffd3, 0x10ffd4, 0x10ffd5, 0x10ffd6, 0x10ffd7, 0x10ffd8, 0, 0, 0, 0, 0,
    0, 0x0a03fa, 0x10ffd9, 0x10ffda, 0x10ffdb, 0x10ffdc, 0x10ffdd, 0x10ffde, 0x10ffdf, 0x10ffe0, 0x10ffe1, 0, 0, 0, 0, 0,
    0, 0x0b07f8, 0x10ffe2, 0x10ffe3, 0x10ffe4, 0x10ffe5, 0x10ffe6, 0x10ffe7, 0x10ffe8, 0x10ffe9, 0x10ffea, 0, 0, 0, 0, 0,
    0, 0x10ffeb, 0x10ffec, 0x10ffed, 0x10ffee, 0x10ffef, 0x10fff0, 0x10fff1, 0x10fff2, 0x10fff3, 0x10fff4, 0, 0, 0, 0, 0,
    0x0b07f9, 0x10fff5, 0x10fff6, 0x10fff7, 0x10fff8, 0x10fff9, 0x10fffa, 0x10fffb, 0x10fffc, 0x10fffd, 0x10fffe, 0, 0, 0, 0, 0,
}, {
    0x020000, 0x020001, 0x030004, 0x04000a, 0x050018, 0x050019, 0x060038, 0x070078, 0x0901f4, 0x0a03f6, 0x0c0ff4, 0, 0, 0, 0, 0,
    0, 0x04000b, 0x060039, 0x0800f6, 0x0901f5, 0x0b07f6, 0x0c0ff5, 0x10ff88, 0x10ff89, 0x10ff8a, 0x10ff8b, 0, 0, 0, 0, 0,
    0, 0x05001a, 0x0800f7, 0x0a03f7, 0x0c0ff6, 0x0f7fc2, 0x10ff8c, 0x10ff8d, 0x10ff8e, 0x10ff8f, 0x10ff90, 0, 0, 0, 0, 0,
    0, 0x05001b, 0x0800f8, 0x0a03f8, 0x0c0ff7, 0x10ff91, 0x10ff92, 0x10ff93, 0x10ff94, 0x10ff95, 0x10ff96, 0, 0, 0, 0, 0,
    0, 0x06003a, 0x0901f6, 0x10ff97, 0x10ff98, 0x10ff99, 0x10ff9a, 0x10ff9b, 0x10ff9c, 0x10ff9d, 0x10ff9e, 0, 0, 0, 0, 0,
    0, 0x06003b, 0x0a03f9, 0x10ff9f, 0x10ffa0, 0x10ffa1, 0x10ffa2, 0x10ffa3, 0x10ffa4, 0x10ffa5, 0x10ffa6, 0, 0, 0, 0, 0,
    0, 0x070079, 0x0b07f7, 0x10ffa7, 0x10ffa8, 0x10ffa9, 0x10ffaa, 0x10ffab, 0x10ffac, 0x10ffad, 0x10ffae, 0, 0, 0, 0, 0,
    0, 0x07007a, 0x0b07f8, 0x10ffaf, 0x10ffb0, 0x10ffb1, 0x10ffb2, 0x10ffb3, 0x10ffb4, 0x10ffb5, 0x10ffb6, 0, 0, 0, 0, 0,
    0, 0x0800f9, 0x10ffb7, 0x10ffb8, 0x10ffb9, 0x10ffba, 0x10ffbb, 0x10ffbc, 0x10ffbd, 0x10ffbe, 0x10ffbf, 0, 0, 0, 0, 0,
    0, 0x0901f7, 0x10ffc0, 0x10ffc1, 0x10ffc2, 0x10ffc3, 0x10ffc4, 0x10ffc5, 0x10ffc6, 0x10ffc7, 0x10ffc8, 0, 0, 0, 0, 0,
    0, 0x0901f8, 0x10ffc9, 0x10ffca, 0x10ffcb, 0x10ffcc, 0x10ffcd, 0x10ffce, 0x10ffcf, 0x10ffd0, 0x10ffd1, 0, 0, 0, 0, 0,
    0, 0x0901f9, 0x10ffd2, 0x10ffd3, 0x10ffd4, 0x10ffd5, 0x10ffd6, 0x10ffd7, 0x10ffd8, 0x10ffd9, 0x10ffda, 0, 0, 0, 0, 0,
    0, 0x0901fa, 0x10ffdb, 0x10ffdc, 0x10ffdd, 0x10ffde, 0x10ffdf, 0x10ffe0, 0x10ffe1, 0x10ffe2, 0x10ffe3, 0, 0, 0, 0, 0,
    0, 0x0b07f9, 0x10ffe4, 0x10ffe5, 0x10ffe6, 0x10ffe7, 0x10ffe8, 0x10ffe9, 0x10ffea, 0x10ffeb, 0x10ffec, 0, 0, 0, 0, 0,
    0, 0x0e3fe0, 0x10ffed, 0x10ffee, 0x10ffef, 0x10fff0, 0x10fff1, 0x10fff2, 0x10fff3, 0x10fff4, 0x10fff5, 0, 0, 0, 0, 0,
    0x0a03fa, 0x0f7fc3, 0x10fff6, 0x10fff7, 0x10fff8, 0x10fff9, 0x10fffa, 0x10fffb, 0x10fffc, 0x10fffd, 0x10fffe, 0, 0, 0, 0, 0,
}};

#define JPG_BLOCK_WORDS 52              // a coded block is at most 22 (DC) + 63 * 26 (AC) = 1660 bits
#define JPG_CHUNK_WORDS 16              // the unstuffed stream is counted and written in chunks of 64 bytes
#define JPG_HDR_WORDS 16

// scratch (int32 words; B = coded blocks = 6 MCUs; every part a multiple of 4 words):
//   [0, 16)            header: u64 0 = bits of the stream before the padding, 1 = its bytes U, 2 = 0xFF bytes among them
//   [16, 16 + 32 B)    int16 coef [B][64], zigzag order, absolute DC (a dummy block: zeros)
//   + 2 B              u64 bit offset per block
//   + 2 B              u32 bits per block (B words used)
//   + 52 B + 16        the unstuffed stream as BIG-ENDIAN 32-bit words (bit b of the stream = bit 31 - b % 32 of word b / 32)
//   + 4 C              C = ceil((52 B + 16) / 16) chunks: u64 0xFF bytes in front of the chunk [C], u32 0xFF bytes of the chunk [C] (2 C words)
static __host__ __device__ inline long jpg_ustream_words(long B) { return JPG_BLOCK_WORDS * B + 16; }
static __host__ __device__ inline long jpg_chunks(long B) { return (jpg_ustream_words(B) + JPG_CHUNK_WORDS - 1) / JPG_CHUNK_WORDS; }
static __host__ __device__ inline long jpg_scratch_words(long B) { return JPG_HDR_WORDS + 32 * B + 4 * B + jpg_ustream_words(B) + 4 * jpg_chunks(B); }

struct JpgGeom {
    int H, W, mw, bw_y, bh_y, ch;       // MCUs per row, Y blocks per row / column, downsampled rows
    long nblk;                          // coded blocks
};

// the blended pixel (ids == null: the frame's)
__device__ __forceinline__ void jpg_pixel(const uint8_t* __restrict__ frame, long ld, const uint8_t* __restrict__ ids, const uint32_t* __restrict__ ctab,
                                          int W, int y, int x, int& r, int& g, int& b) {
    const uint8_t* px = frame + (long)y * ld + 3l * x;
    r = px[0]; g = px[1]; b = px[2];
    if (ids) {
        const uint32_t id = ids[(long)y * W + x];
        if (id) {
            const uint32_t c = ctab[id];
            r = (r + (int)(c & 255u)) >> 1;
            g = (g + (int)((c >> 8) & 255u)) >> 1;
            b = (b + (int)((c >> 16) & 255u)) >> 1;
        }
    }
}

#define JPG_DESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))

// jfdctint.c, one pass over 8 values.  32-bit: the inputs of pass 1 are |d| <= 128, its outputs |d| <= 4096; in pass 2 a sum of two
// is <= 8192, of four <= 32768, and the largest intermediate is tmp6 * 25172 + z2 + z3 <= 8192 * 25172 + 16384 * 20995 + 16384 * 16069
// + 32768 * 9633 < 1.13e9 < 2^31 (tests/jpeg_enc_ref.py asserts the range on everything it encodes).
template <bool FIRST>
__device__ __forceinline__ void jpg_fdct8(int* d) {
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = FIRST ? 13 - 2 : 13 + 2;
    if (FIRST) { d[0] = (t10 + t11) << 2; d[4] = (t10 - t11) << 2; }
    else { d[0] = JPG_DESCALE(t10 + t11, 2); d[4] = JPG_DESCALE(t10 - t11, 2); }
    int z1 = (t12 + t13) * 4433;
    d[2] = JPG_DESCALE(z1 + t13 * 6270, n);
    d[6] = JPG_DESCALE(z1 + t12 * -15137, n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int m4 = t4 * 2446, m5 = t5 * 16819, m6 = t6 * 25172, m7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    d[7] = JPG_DESCALE(m4 + z1 + z3, n);
    d[5] = JPG_DESCALE(m5 + z2 + z4, n);
    d[3] = JPG_DESCALE(m6 + z2 + z3, n);
    d[1] = JPG_DESCALE(m7 + z1 + z4, n);
}

__device__ __forceinline__ bool jpg_is_dummy(long g, const JpgGeom& G) {
    const int k = (int)(g % 6);
    if (k >= 4) return false;
    const long mcu = g / 6;
    const int my = (int)(mcu / G.mw), mx = (int)(mcu % G.mw);
    return 2 * my + (k >> 1) >= G.bh_y || 2 * mx + (k & 1) >= G.bw_y;
}

// A: 32 coded blocks per workgroup, 8 threads per block: thread (b, r) gathers row r (blend, colour conversion, downsampling, edge
// replication) and runs the row pass, then column r's pass, quantises and puts the column into zigzag order in LDS.
extern "C" __global__ __launch_bounds__(256) void jpg_transform_kernel(const uint8_t* __restrict__ frame, long ld, const uint8_t* __restrict__ ids,
                                                                       const uint32_t* __restrict__ ctab, const uint16_t* __restrict__ qt, JpgGeom G,
                                                                       int16_t* __restrict__ coef) {
    __shared__ int tile[32][8][9];
    __shared__ __attribute__((aligned(16))) int16_t outz[32][64];
    __shared__ int q[2][64];
    const int t = threadIdx.x, b = t >> 3, r = t & 7;
    if (t < 128) { const int v = qt[t]; q[t >> 6][t & 63] = (v < 1 ? 1 : v) << 3; }
    const long g = (long)blockIdx.x * 32 + b;
    const bool valid = g < G.nblk;
    const int k = valid ? (int)(g % 6) : 0;
    const long mcu = valid ? g / 6 : 0;
    const int my = (int)(mcu / G.mw), mx = (int)(mcu % G.mw);
    const bool work = valid && !jpg_is_dummy(g, G);
    int d[8];
    if (work) {
        const int H = G.H, W = G.W;
        if (k < 4) {
            const int y = min((2 * my + (k >> 1)) * 8 + r, H - 1), x0 = (2 * mx + (k & 1)) * 8;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                int R, Gn, B;
                jpg_pixel(frame, ld, ids, ctab, W, y, min(x0 + c, W - 1), R, Gn, B);
                d[c] = ((19595 * R + 38470 * Gn + 7471 * B + 32768) >> 16) - 128;
            }
        } else {
            const int cy = min(my * 8 + r, G.ch - 1), y0 = min(2 * cy, H - 1), y1 = min(2 * cy + 1, H - 1);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int cx = mx * 8 + c, xa = min(2 * cx, W - 1), xb = min(2 * cx + 1, W - 1);
                int s = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int R, Gn, B;
                    jpg_pixel(frame, ld, ids, ctab, W, (j & 2) ? y1 : y0, (j & 1) ? xb : xa, R, Gn, B);
                    s += k == 4 ? (-11059 * R - 21709 * Gn + 32768 * B + (128 << 16) + 32767) >> 16
                                : (32768 * R - 27439 * Gn - 5329 * B + (128 << 16) + 32767) >> 16;
                }
                d[c] = ((s + 1 + (c & 1)) >> 2) - 128;
            }
        }
        jpg_fdct8<true>(d);
#pragma unroll
        for (int c = 0; c < 8; ++c) tile[b][r][c] = d[c];
    }
    __syncthreads();
    if (work) {
#pragma unroll
        for (int u = 0; u < 8; ++u) d[u] = tile[b][u][r];
        jpg_fdct8<false>(d);
        const int* qq = q[k >= 4];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int nat = u * 8 + r, div = qq[nat], a = d[u] < 0 ? -d[u] : d[u], m = (a + (div >> 1)) / div;
            outz[b][JPG_ZZ_OF_NATURAL[nat]] = (int16_t)(d[u] < 0 ? -m : m);
        }
    } else if (valid) {
#pragma unroll
        for (int c = 0; c < 8; ++c) outz[b][r * 8 + c] = 0;
    }
    __syncthreads();
    if (valid) ((uint4*)(coef + g * 64))[r] = ((const uint4*)outz[b])[r];
}

// DC of the block of g's component that was coded last before g (0 at the start of the scan); g is not a dummy block
__device__ __forceinline__ int jpg_pred_dc(const int16_t* __restrict__ coef, long g, const JpgGeom& G) {
    const int k = (int)(g % 6);
    if (k >= 4) return g >= 6 ? (int)coef[(g - 6) * 64] : 0;
    for (long j = g - 1; j >= 0; --j)             // (block 0 of an MCU is never a dummy: at most six steps)
        if (j % 6 < 4 && !jpg_is_dummy(j, G)) return (int)coef[j * 64];
    return 0;
}

// One wave per coded block, lane z = zigzag index: the lane's Huffman code + magnitude bits (lane 0 the DC difference, a lane with a
// nonzero AC coefficient its ZRLs, code and bits -- the run comes from the ballot of the nonzero lanes --, lane 63 the EOB when the
// last coefficient is zero), MSB first in `bits`, `len` <= 59; -> the lane's bit position inside the block and the block's bits.
__device__ __forceinline__ void jpg_block_code(const int16_t* __restrict__ coef, long g, const JpgGeom& G, int lane, uint64_t& bits, int& len,
                                               int& pos, int& total) {
    const int chroma = (int)(g % 6) >= 4;
    int v = 0;
    if (!jpg_is_dummy(g, G)) {
        v = (int)coef[g * 64 + lane];
        if (lane == 0) v -= jpg_pred_dc(coef, g, G);
    }
    const uint64_t nz = __ballot(lane > 0 && v != 0);
    // (8-bit samples give DC differences of at most 11 bits and AC coefficients of at most 10; the clamp only bounds the block's bits
    // -- 22 + 63 * 26 = 1660 -- for tables the caller got wrong)
    const int a = v < 0 ? -v : v, cat = min(a ? 32 - __clz(a) : 0, lane == 0 ? 11 : 10);
    const uint32_t mag = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u);
    bits = 0;
    len = 0;
    if (lane == 0) {
        const uint32_t e = JPG_DC[chroma][cat];
        bits = ((uint64_t)(e & 0xffffu) << cat) | mag;
        len = (int)(e >> 16) + cat;
    } else if (v != 0) {
        const uint64_t below = nz & ((1ull << lane) - 1ull);
        const int prev = below ? 63 - __clzll((long long)below) : 0, run = lane - prev - 1;
        const uint32_t e = JPG_AC[chroma][((run & 15) << 4) | cat], zrl = JPG_AC[chroma][0xF0];
        const int zs = (int)(zrl >> 16), size = (int)(e >> 16);
        for (int i = 0; i < (run >> 4); ++i) bits = (bits << zs) | (zrl & 0xffffu);
        bits = (((bits << size) | (e & 0xffffu)) << cat) | mag;
        len = (run >> 4) * zs + size + cat;
    } else if (lane == 63) {
        const uint32_t e = JPG_AC[chroma][0];
        bits = e & 0xffffu;
        len = (int)(e >> 16);
    }
    int incl = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    pos = incl - len;
    total = __shfl(incl, 63, 64);
}

// B: bits per block
extern "C" __global__ __launch_bounds__(256) void jpg_count_kernel(const int16_t* __restrict__ coef, JpgGeom G, uint32_t* __restrict__ nbits) {
    const int lane = threadIdx.x & 63;
    const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= G.nblk) return;
    uint64_t bits;
    int len, pos, total;
    jpg_block_code(coef, g, G, lane, bits, len, pos, total);
    if (lane == 0) nbits[g] = (uint32_t)total;
}

// C: one workgroup, fixed order: exclusive scan of n 32-bit counts into 64-bit offsets; hdr[slot] = the sum
__device__ __forceinline__ uint64_t jpg_scan(const uint32_t* __restrict__ cnt, long n, unsigned long long* __restrict__ off, uint32_t* part,
                                             unsigned long long* carry_s) {
    const int t = threadIdx.x;
    if (t == 0) *carry_s = 0ull;
    __syncthreads();
    for (long base = 0; base < n; base += 1024) {
        const long i = base + t;
        const uint32_t v = i < n ? cnt[i] : 0u;
        part[t] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {                     // inclusive scan (1024 counts of < 2^22 each fit 32 bits)
            const uint32_t add = t >= o ? part[t - o] : 0u;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        const unsigned long long carry = *carry_s;
        if (i < n) off[i] = carry + part[t] - v;
        __syncthreads();
        if (t == 1023) *carry_s = carry + part[1023];
        __syncthreads();
    }
    return *carry_s;
}

extern "C" __global__ __launch_bounds__(1024) void jpg_scan_bits_kernel(const uint32_t* __restrict__ nbits, long nblk, unsigned long long* __restrict__ off,
                                                                         unsigned long long* __restrict__ hdr) {
    __shared__ uint32_t part[1024];
    __shared__ unsigned long long carry_s;
    const uint64_t T = jpg_scan(nbits, nblk, off, part, &carry_s);
    if (threadIdx.x == 0) { hdr[0] = T; hdr[1] = (T + 7) >> 3; hdr[2] = 0; }
}

// D: clears the words the unstuffed stream will use (and one chunk behind them: the counting kernel reads whole chunks)
extern "C" __global__ __launch_bounds__(256) void jpg_clear_kernel(const unsigned long long* __restrict__ hdr, uint32_t* __restrict__ ustream) {
    const long n = (long)((hdr[1] + 3) >> 2) + JPG_CHUNK_WORDS;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) ustream[i] = 0u;
}

// `len` bits (1 .. 59, MSB first) at bit `pos` of a block's buffer of big-endian words
__device__ __forceinline__ void jpg_place(uint32_t* buf, uint64_t bits, int len, int pos) {
    const uint64_t V = bits << (64 - len);
    const int w0 = pos >> 5, s = pos & 31;
    const uint64_t hi = V >> s;
    const uint32_t a0 = (uint32_t)(hi >> 32), a1 = (uint32_t)hi, a2 = s ? (uint32_t)((V << (64 - s)) >> 32) : 0u;
    if (a0) atomicOr(buf + w0, a0);
    if (a1) atomicOr(buf + w0 + 1, a1);
    if (a2) atomicOr(buf + w0 + 2, a2);
}

// E: one wave per coded block: the block's bits are put together in LDS, then shifted to the block's offset.  Interior words have one
// owner (plain stores); the first and the last word are shared with the neighbours and OR-ed in with a vector atomic.  The wave of the
// last block appends the 1-bits that fill the last byte.
extern "C" __global__ __launch_bounds__(256) void jpg_emit_kernel(const int16_t* __restrict__ coef, JpgGeom G, const unsigned long long* __restrict__ off,
                                                                   uint32_t* __restrict__ ustream) {
    __shared__ uint32_t buf[4][JPG_BLOCK_WORDS + 4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long g = (long)blockIdx.x * 4 + w;
    const bool active = g < G.nblk;
    if (lane < JPG_BLOCK_WORDS + 4) buf[w][lane] = 0u;
    __syncthreads();
    uint64_t o = 0;
    int total = 0;
    if (active) {
        uint64_t bits;
        int len, pos;
        jpg_block_code(coef, g, G, lane, bits, len, pos, total);
        o = off[g];
        if (len > 0) jpg_place(buf[w], bits, len, pos);
        if (g == G.nblk - 1) {
            const int pad = (int)((0 - (o + (uint64_t)total)) & 7u);
            if (lane == 0 && pad) jpg_place(buf[w], (1u << pad) - 1u, pad, total);
            total += pad;
        }
    }
    __syncthreads();
    if (!active || total == 0) return;
    const uint64_t W0 = o >> 5;
    const int sh = (int)(o & 31u), last = (sh + total - 1) >> 5;
    for (int j = lane; j <= last; j += 64) {
        const uint32_t cur = j < JPG_BLOCK_WORDS + 4 ? buf[w][j] : 0u, prev = (j > 0 && j - 1 < JPG_BLOCK_WORDS + 4) ? buf[w][j - 1] : 0u;
        const uint32_t val = sh ? (cur >> sh) | (prev << (32 - sh)) : cur;
        if (j == 0 || j == last) { if (val) atomicOr(ustream + W0 + j, val); }
        else ustream[W0 + j] = val;
    }
}

__device__ __forceinline__ uint32_t jpg_ff_bytes(uint32_t v) {
    return ((v >> 24) == 255u) + (((v >> 16) & 255u) == 255u) + (((v >> 8) & 255u) == 255u) + ((v & 255u) == 255u);
}

// F: 0xFF bytes per chunk of the unstuffed stream (the words behind its last byte are zero)
extern "C" __global__ __launch_bounds__(256) void jpg_ff_count_kernel(const unsigned long long* __restrict__ hdr, const uint32_t* __restrict__ ustream,
                                                                       uint32_t* __restrict__ cnt) {
    const long c = (long)blockIdx.x * 256 + threadIdx.x, nchunk = (long)((hdr[1] + 63) >> 6);
    if (c >= nchunk) return;
    const uint4* src = (const uint4*)(ustream + c * JPG_CHUNK_WORDS);
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < JPG_CHUNK_WORDS / 4; ++k) {
        const uint4 v = src[k];
        n += jpg_ff_bytes(v.x) + jpg_ff_bytes(v.y) + jpg_ff_bytes(v.z) + jpg_ff_bytes(v.w);
    }
    cnt[c] = n;
}

// G: one workgroup: the chunks' byte offsets after stuffing, the capacity check and the status block
//    status = {stream bytes (saturating at 2^31 - 1), 0, error bits (1: the stream does not fit the capacity; nothing is written then), 0}
extern "C" __global__ __launch_bounds__(1024) void jpg_scan_ff_kernel(const uint32_t* __restrict__ cnt, unsigned long long* __restrict__ ffoff,
                                                                       unsigned long long* __restrict__ hdr, int cap, int* __restrict__ status) {
    __shared__ uint32_t part[1024];
    __shared__ unsigned long long carry_s;
    const long nchunk = (long)((hdr[1] + 63) >> 6);
    const uint64_t ff = jpg_scan(cnt, nchunk, ffoff, part, &carry_s);
    if (threadIdx.x == 0) {
        const uint64_t len = hdr[1] + ff;
        hdr[2] = ff;
        status[0] = len > 0x7fffffffull ? 0x7fffffff : (int)len;
        status[1] = 0;
        status[2] = len <= (uint64_t)cap ? 0 : 1;
        status[3] = 0;
    }
}

// H: one thread per chunk writes its bytes, a zero behind every 0xFF
extern "C" __global__ __launch_bounds__(256) void jpg_write_kernel(const unsigned long long* __restrict__ hdr, const uint32_t* __restrict__ ustream,
                                                                    const unsigned long long* __restrict__ ffoff, const int* __restrict__ status,
                                                                    uint8_t* __restrict__ out) {
    if (status[2] != 0) return;
    const long c = (long)blockIdx.x * 256 + threadIdx.x, U = (long)hdr[1], nchunk = (U + 63) >> 6;
    if (c >= nchunk) return;
    const uint32_t* src = ustream + c * JPG_CHUNK_WORDS;
    uint8_t* dst = out + c * 64 + (long)ffoff[c];
    const int n = (int)min(64l, U - c * 64);
    for (int j = 0; j < n; ++j) {
        const uint32_t byte = (src[j >> 2] >> (24 - 8 * (j & 3))) & 255u;
        *dst++ = (uint8_t)byte;
        if (byte == 255u) *dst++ = 0;
    }
}

// PROB_TO_ID flags == 128 (slots: include/cutie_hip.h, ABI 11)
int launch_jpeg_encode(const cutie_op* op, hipStream_t s) {
    const uint64_t* p = op->p;
    const int H = op->i[1], W = op->i[2], ld = op->i[4], cap = op->i[7];
    if (H < 1 || W < 1) { cutie_set_error("jpeg encode: empty shape (H, W >= 1)"); return -2; }
    if (H > 65535 || W > 65535) { cutie_set_error("jpeg encode: %d x %d, a JPEG is at most 65535 wide and high", H, W); return -2; }
    if ((long)H * W >= (1l << 31)) { cutie_set_error("jpeg encode: %d x %d exceeds 2^31 pixels", H, W); return -2; }
    if (cap < 0) { cutie_set_error("jpeg encode: negative capacity"); return -2; }
    if (!p[0] || (!p[3] && cap > 0) || !p[4] || !p[5] || !p[7] || (p[2] && !p[6])) {
        cutie_set_error("jpeg encode: needs the frame (p0), the stream (p3), the status (p4), the scratch (p5), the quant tables (p7) and, with an id plane (p2), the colour table (p6)");
        return -2;
    }
    if ((p[4] & 3) || (p[5] & 15) || (p[6] & 3) || (p[7] & 1)) {
        cutie_set_error("jpeg encode: status and colour table 4-byte aligned, quant tables 2-byte aligned, scratch 16-byte aligned");
        return -2;
    }
    if ((long)ld < 3l * W) { cutie_set_error("jpeg encode: frame row stride of %d bytes, needs 3 W = %ld", ld, 3l * W); return -2; }
    JpgGeom G;
    G.H = H; G.W = W;
    G.mw = (W + 15) / 16;
    G.bw_y = (W + 7) / 8; G.bh_y = (H + 7) / 8;
    G.ch = (H + 1) / 2;
    G.nblk = 6l * G.mw * ((H + 15) / 16);
    const long B = G.nblk, need = jpg_scratch_words(B);
    if ((long)op->i[8] < need) { cutie_set_error("jpeg encode: scratch of %d words, needs %ld", op->i[8], need); return -2; }
    int* base = (int*)p[5];
    unsigned long long* hdr = (unsigned long long*)base;
    int16_t* coef = (int16_t*)(base + JPG_HDR_WORDS);
    unsigned long long* off = (unsigned long long*)(base + JPG_HDR_WORDS + 32 * B);
    uint32_t* nbits = (uint32_t*)(base + JPG_HDR_WORDS + 34 * B);
    uint32_t* ustream = (uint32_t*)(base + JPG_HDR_WORDS + 36 * B);
    const long C = jpg_chunks(B);
    unsigned long long* ffoff = (unsigned long long*)(ustream + jpg_ustream_words(B));
    uint32_t* cnt = (uint32_t*)(ffoff + C);
    const unsigned gb = (unsigned)((B + 3) / 4), gc = (unsigned)((C + 255) / 256);
    hipLaunchKernelGGL(jpg_transform_kernel, dim3((unsigned)((B + 31) / 32)), dim3(256), 0, s, (const uint8_t*)p[0], (long)ld, (const uint8_t*)p[2],
                       (const uint32_t*)p[6], (const uint16_t*)p[7], G, coef);
    hipLaunchKernelGGL(jpg_count_kernel, dim3(gb), dim3(256), 0, s, (const int16_t*)coef, G, nbits);
    hipLaunchKernelGGL(jpg_scan_bits_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t*)nbits, B, off, hdr);
    hipLaunchKernelGGL(jpg_clear_kernel, dim3((unsigned)min(256l, (jpg_ustream_words(B) + 255) / 256)), dim3(256), 0, s, (const unsigned long long*)hdr, ustream);
    hipLaunchKernelGGL(jpg_emit_kernel, dim3(gb), dim3(256), 0, s, (const int16_t*)coef, G, (const unsigned long long*)off, ustream);
    hipLaunchKernelGGL(jpg_ff_count_kernel, dim3(gc), dim3(256), 0, s, (const unsigned long long*)hdr, (const uint32_t*)ustream, cnt);
    hipLaunchKernelGGL(jpg_scan_ff_kernel, dim3(1), dim3(1024), 0, s, (const uint32_t*)cnt, ffoff, hdr, cap, (int*)p[4]);
    hipLaunchKernelGGL(jpg_write_kernel, dim3(gc), dim3(256), 0, s, (const unsigned long long*)hdr, (const uint32_t*)ustream, (const unsigned long long*)ffoff,
                       (const int*)p[4], (uint8_t*)p[3]);
    return (int)hipGetLastError();
}
