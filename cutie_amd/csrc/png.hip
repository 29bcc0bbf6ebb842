// PROB_TO_ID flags&8 (ABI 7): the zlib stream of a PNG's IDAT chunk, made on the device from the uint8 object-id plane [H, W]
// (ResultSaver egress='device', cutie_amd/inference/utils/results_utils.py; container: cutie_amd/inference/utils/png.py).
//
// The inflated data is the PNG-filtered image: every row is the filter byte 0 ("None") followed by its W ids, L = W + 1 bytes.  ONE DEFLATE
// block with the fixed Huffman codes (RFC 1951 3.2.6) holds all rows.  Tokens never cross a row, so rows are independent:
//   at byte i of a row:  u = number of bytes from i on that equal the byte one row up (distance L; 0 in the first row)
//                        r = number of bytes from i on that equal their left neighbour inside the row (distance 1; 0 at i = 0)
//                        n = max(u, r);  n < 3: literal, one byte.  Else a match of take(n) bytes, distance L if u >= r, else 1, where
//                        take(n) = n for n <= 258, n - 3 for n = 259 | 260 (so that no 1- or 2-byte rest is left), else 258.
// Result masks are a few runs per row that mostly repeat the row above: a 480p row is typically four matches, ~10 bytes.
// tests/png_ref.py is the same rule in numpy; the bytes are equal.
//
// Three launches (a grid-wide dependency lies between them: a row's bit offset is the sum of the bit counts of all rows above it):
//   A  png_rows_kernel    one wave per row: the row and the one above it are compared 64 bytes per step, the equal-up / equal-left flags go
//                         to LDS as bit masks (ballot), lane 0 walks the masks run by run (ctz, not byte by byte) and writes the row's bits,
//                         starting at bit 0, to the row's slice of the scratch; all lanes sum the row's Adler-32 partials meanwhile.
//   B  png_scan_kernel    one block: exclusive scan of the rows' bit counts, Adler-32 of the whole image from the partials (Adler composes:
//                         all sums are integers mod 65521, so the order of the additions does not matter), length check against the
//                         capacity, clears exactly the words the stream will use, writes header, trailer and the status block.
//   C  png_emit_kernel    one wave per row: shifts the row's bits to their offset.  Interior words have one owner (plain stores); the first
//                         and the last word of a row are shared with its neighbours and are OR-ed in with a vector atomic.
// The same plane gives the same bytes whatever the launch shape: nothing depends on the order in which rows arrive.
#include "common.h"
#include "deflate_enc.h"            // bit writer, symbols, fixed codes, run lengths, the scan body and the shift-out, shared with png_photo.hip

static __host__ __device__ inline int png_row_words(int L) { return (9 * L + 31) / 32 + 2; }      // fixed codes: at most 9 bits per byte

__device__ __forceinline__ void png_literal(DeBits& b, uint32_t v) {
    const uint32_t e = de_fixed_lit(v);
    b.put(e & 0xffffu, (int)(e >> 16));
}

// length 3..258 under the fixed codes, then the distance code prepared by the caller
__device__ __forceinline__ void png_match(DeBits& b, int len, uint32_t dbits, int dn) {
    int sym, eb;
    uint32_t extra;
    de_len_sym(len, sym, eb, extra);
    const uint32_t e = de_fixed_len(sym);
    const int cn = (int)(e >> 16);
    b.put((e & 0xffffu) | (extra << cn), cn + eb);  // <= 13 bits
    b.put(dbits, dn);                               // <= 18 bits
}

// distance symbol under the fixed 5-bit code + extra bits as one LSB-first field
__device__ __forceinline__ void png_dist(int dist, uint32_t& bits, int& n) {
    int sym, eb;
    uint32_t extra;
    de_dist_sym(dist, sym, eb, extra);
    bits = de_rev((uint32_t)sym, 5) | (extra << 5);
    n = 5 + eb;
}

// A: grid = H rows, block = one wave.  info[r] = {bits, sum of bytes mod 65521, sum of (L - j) * byte_j mod 65521, -}
extern "C" __global__ __launch_bounds__(64) void png_rows_kernel(const uint8_t* __restrict__ ids, int H, int W, int4* __restrict__ info,
                                                                  uint32_t* __restrict__ scratch, int stride) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int r = blockIdx.x, lane = threadIdx.x;
    const int L = W + 1, nmask = (L + 63) >> 6;
    uint64_t* mu = (uint64_t*)lds;                 // equal to the byte one row up
    uint64_t* me = mu + nmask + 1;                 // equal to the byte on the left
    uint8_t* cur = (uint8_t*)(me + nmask + 1);     // the filtered row
    const uint8_t* row = ids + (long)r * W;
    uint64_t S = 0, T = 0;
    for (int base = 0; base < nmask * 64; base += 64) {
        const int i = base + lane;
        const bool in = i < L;
        const uint32_t c = (in && i > 0) ? row[i - 1] : 0u;
        const uint32_t left = (in && i > 1) ? row[i - 2] : 0u;
        const uint32_t up = (in && i > 0 && r > 0) ? row[i - 1 - (long)W] : 0u;
        const uint64_t bu = __ballot(in && r > 0 && c == up), be = __ballot(in && i > 0 && c == left);
        if (lane == 0) { mu[base >> 6] = bu; me[base >> 6] = be; }
        cur[i] = (uint8_t)c;
        S += c;
        T += (uint64_t)(L - i) * c;
    }
    if (lane == 0) mu[nmask] = me[nmask] = 0;
    for (int o = 32; o > 0; o >>= 1) {
        S += __shfl_xor((unsigned long long)S, o, 64);
        T += __shfl_xor((unsigned long long)T, o, 64);
    }
    __syncthreads();
    if (lane != 0) return;
    uint32_t dbits1, dbitsL;
    int dn1, dnL;
    png_dist(1, dbits1, dn1);
    png_dist(L, dbitsL, dnL);
    DeBits b{scratch + (long)r * stride, 0ull, 0, 0};
    int i = 0;
    while (i < L) {
        const int u = de_run<0>(mu, i, nmask), e = i > 0 ? de_run<0>(me, i, nmask) : 0;
        const int n = u >= e ? u : e;
        if (n < 3) {
            const uint32_t v = cur[i];
            png_literal(b, v);
            i += 1;
            continue;
        }
        const int take = de_take(n);
        if (u >= e) png_match(b, take, dbitsL, dnL);
        else png_match(b, take, dbits1, dn1);
        i += take;
    }
    info[r] = make_int4(b.finish(), (int)(S % DE_ADLER), (int)(T % DE_ADLER), 0);
}

// B: one block (de_scan): 2 header bytes, 3 bits block header, the rows, 7 bits end-of-block (code 0: the cleared buffer holds it already).
// Word 0: the zlib header (32K window, no dictionary), then BFINAL = 1, BTYPE = 01
extern "C" __global__ __launch_bounds__(1024) void png_scan_kernel(int4* __restrict__ info, int H, int W, uint8_t* __restrict__ out, int cap,
                                                                    int* __restrict__ status) {
    de_scan(info, H, W + 1, 16u + 3u, 7u, 0x78u | (0x01u << 8) | (3u << 16), out, cap, status);
}

// C: grid = H rows, block = one wave
extern "C" __global__ __launch_bounds__(64) void png_emit_kernel(const int4* __restrict__ info, int H, const uint32_t* __restrict__ scratch,
                                                                  int stride, uint32_t* __restrict__ out, const int* __restrict__ status) {
    if (status[2] != 0) return;
    const int r = blockIdx.x, lane = threadIdx.x;
    const int4 v = info[r];
    const uint32_t nbits = (uint32_t)v.x, off = 19u + (uint32_t)v.w;
    if (nbits == 0) return;
    de_shift_out(scratch + (long)r * stride, (nbits + 31) >> 5, nbits, off, out, lane);
}

// PROB_TO_ID flags&8.  p2 = ids u8 [H, W] (H, W: the plane as stored, i.e. the output geometry of the id stage), p3 = stream, i7 = capacity,
// p4 = status int32 [4], p5 = scratch int32 [i8]
int launch_png_deflate(const cutie_op* op, int H, int W, hipStream_t s) {
    const uint64_t* p = op->p;
    const int cap = op->i[7] & ~3;
    const long L = (long)W + 1;
    if (H < 1 || W < 1 || W > 32767) { cutie_set_error("png deflate: H >= 1 and 1 <= W <= 32767 (the distance of a row is W + 1)"); return -2; }
    if (L * H * 9 + 64 >= (1l << 31)) { cutie_set_error("png deflate: %d x %d exceeds 2^31 stream bits", H, W); return -2; }
    // (a capacity below 4 bytes holds no stream: the overflow bit is set and p3, which may then be null -- an empty buffer -- is never touched)
    if (!p[2] || (!p[3] && cap > 0) || !p[4] || !p[5]) { cutie_set_error("png deflate: needs the id plane (p2), the stream (p3), the status (p4) and the scratch (p5)"); return -2; }
    if ((p[3] & 3) || (p[4] & 3) || (p[5] & 15)) { cutie_set_error("png deflate: stream and status 4-byte aligned, scratch 16-byte aligned"); return -2; }
    if (cap < 0) { cutie_set_error("png deflate: negative capacity"); return -2; }
    const int stride = png_row_words((int)L);
    const long need = 4l * H + (long)H * stride;
    if ((long)op->i[8] < need) { cutie_set_error("png deflate: scratch of %d words, needs %ld", op->i[8], need); return -2; }
    int4* info = (int4*)p[5];
    uint32_t* scratch = (uint32_t*)p[5] + 4l * H;
    const int nmask = (int)((L + 63) >> 6);
    const size_t lds = (size_t)(2 * (nmask + 1)) * 8 + (size_t)nmask * 64;
    hipLaunchKernelGGL(png_rows_kernel, dim3(H), dim3(64), lds, s, (const uint8_t*)p[2], H, W, info, scratch, stride);
    hipLaunchKernelGGL(png_scan_kernel, dim3(1), dim3(1024), 0, s, info, H, W, (uint8_t*)p[3], cap, (int*)p[4]);
    hipLaunchKernelGGL(png_emit_kernel, dim3(H), dim3(64), 0, s, (const int4*)info, H, (const uint32_t*)scratch, stride, (uint32_t*)p[3], (const int*)p[4]);
    return (int)hipGetLastError();
}
