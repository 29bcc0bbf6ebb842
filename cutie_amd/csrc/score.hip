// PROB_TO_ID flags == 64 (ABI 10): the integers behind DAVIS J&F of a predicted uint8 id plane against a ground-truth one, per listed
// object -- region overlap (J) and the boundary match (F) of davis2017-evaluation (metrics.py db_eval_iou / db_eval_boundary, utils.py
// seg2bmap), counted on the device so that only 8 integers per (frame, object) ever leave it (the float arithmetic on them:
// cutie_amd/inference/utils/davis_metrics.py; the numpy / scipy model of these counts: tests/jf_ref.py).
//
// Object k is scored on the binary masks P = (pred == objs[k]) and G = (gt == objs[k]).  Its boundary map, seg2bmap at equal size:
//   b = (s ^ e) | (s ^ so) | (s ^ se)   with the east, south and south-east neighbours; a neighbour outside the image is replaced by s
// itself -- which is the package's "last row: s ^ e only, last column: s ^ so only, bottom-right pixel: 0".  A boundary pixel of A at
// (y, x) is matched when B has a boundary pixel at (y + dy, x + dx), inside the image, with dy^2 + dx^2 <= r^2: B dilated by disk(r),
// nothing outside the image (cv2.dilate / skimage's disk).
//
// A row of a bit plane is ceil(W / 64) 64-bit words, bit i of word w = column 64 w + i: one __ballot of a wave.  Three launches:
//   1  jf_zero_kernel     counts[n][8] = 0 (the launch WRITES the table)
//   2  jf_pack_kernel     a wave takes 64 columns of one row: the four neighbours of both planes once, then per object four ballots
//                         (P, G and their boundary bits): columns 0 1 2 3 6 7 are popcounts of those words; the two boundary words go to
//                         the scratch [2][n][H][ceil(W / 64)].  64 columns of background in both planes (most of a frame) take a shortcut.
//   3  jf_match_kernel    a thread takes one boundary word A of one object and one direction (pred against gt: column 4, gt against
//                         pred: column 5); a word without boundary pixels -- nearly all -- leaves at once.  Otherwise
//                         dilated = OR over dy of hdilate(row y + dy of B, h(dy)), h(dy) = isqrt(r^2 - dy^2) from a host table, rows from the
//                         nearest outwards, until every bit of A is matched.  hdilate of a word needs its two neighbours: the word's own
//                         bits are smeared by shift-or doubling, the left neighbour gives the columns up to (its highest bit within
//                         h) + h, the right one those from (its lowest bit within h) - h.  popcount(A & dilated) is the thread's share.
// Every count is a sum of popcounts gathered with integer atomics (LDS first, one global add per block, object and column): the result
// depends on the planes, the object list and r alone, not on launch shape or timing.
#include "common.h"

#define JF_MAX_RADIUS 40                 // CUTIE_JF_MAX_RADIUS (include/cutie_hip.h): a disk row reaches the neighbouring word only (< 64)
#define JF_WORDS_PER_WAVE 4              // launch 2: words per wave, 16 per block

struct JfSpans { unsigned char h[JF_MAX_RADIUS + 1]; };      // h[|dy|] = isqrt(r^2 - dy^2)

__global__ __launch_bounds__(256) void jf_zero_kernel(int* __restrict__ counts, int n8) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < n8) counts[idx] = 0;
}

// launch 2: grid = ceil(H * WW / 16)
__global__ __launch_bounds__(256) void jf_pack_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, int H, int W, int WW,
                                                      const int* __restrict__ objs, int n, unsigned long long* __restrict__ bnd, int* __restrict__ counts) {
    __shared__ int lcnt[256 * 8];
    __shared__ int objs_s[256];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int idx = t; idx < n * 8; idx += 256) lcnt[idx] = 0;
    {
        const int v = t < n ? objs[t] : -1;
        objs_s[t] = (v >= 1 && v <= 254) ? v : -1;            // anything else is an absent object: all counts 0, J = F = 1 by convention
    }
    __syncthreads();
    const long NW = (long)H * WW;                             // words of one bit plane
    for (int q = 0; q < JF_WORDS_PER_WAVE; ++q) {
        const long g = ((long)blockIdx.x * 4 + w) * JF_WORDS_PER_WAVE + q;
        if (g >= NW) break;                                   // (uniform in the wave)
        const int y = (int)(g / WW), x = (int)(g % WW) * 64 + lane;
        int p00 = 0, p01 = 0, p10 = 0, p11 = 0, g00 = 0, g01 = 0, g10 = 0, g11 = 0;
        const bool in = x < W;
        if (in) {
            const long at = (long)y * W + x;
            const bool east = x + 1 < W, south = y + 1 < H;
            p00 = pred[at];
            g00 = gt[at];
            p01 = east ? pred[at + 1] : p00;
            g01 = east ? gt[at + 1] : g00;
            p10 = south ? pred[at + W] : p00;
            g10 = south ? gt[at + W] : g00;
            p11 = (east && south) ? pred[at + W + 1] : p00;
            g11 = (east && south) ? gt[at + W + 1] : g00;
        }
        if (__ballot((p00 | p01 | p10 | p11 | g00 | g01 | g10 | g11) != 0) == 0ull) {       // background only: no object has anything here
            for (int k = lane; k < n; k += 64) {
                bnd[(long)k * NW + g] = 0ull;
                bnd[((long)n + k) * NW + g] = 0ull;
            }
            continue;
        }
        for (int k = 0; k < n; ++k) {
            const int id = objs_s[k];
            const bool sp = in && p00 == id, sg = in && g00 == id;
            const bool bp = sp != (p01 == id) || sp != (p10 == id) || sp != (p11 == id);
            const bool bg = sg != (g01 == id) || sg != (g10 == id) || sg != (g11 == id);
            const unsigned long long mp = __ballot(sp), mg = __ballot(sg), wp = __ballot(in && bp), wg = __ballot(in && bg);
            if (lane == 0) {
                bnd[(long)k * NW + g] = wp;
                bnd[((long)n + k) * NW + g] = wg;
            }
            int v = 0, col = lane;
            switch (lane) {
                case 0: v = __popcll(mp & mg); break;
                case 1: v = __popcll(mp | mg); break;
                case 2: v = __popcll(wp); break;
                case 3: v = __popcll(wg); break;
                case 4: v = __popcll(mp); col = 6; break;
                case 5: v = __popcll(mg); col = 7; break;
                default: break;
            }
            if (lane < 6 && v) atomicAdd(&lcnt[k * 8 + col], v);
        }
    }
    __syncthreads();
    for (int idx = t; idx < n * 8; idx += 256)
        if (lcnt[idx]) atomicAdd(counts + idx, lcnt[idx]);
}

// bits of x moved up by 0 .. h columns (h < 64), ORed: shift-or doubling
__device__ __forceinline__ unsigned long long jf_smear_up(unsigned long long x, int h) {
    int s = 1;
    while (2 * s <= h + 1) { x |= x << s; s *= 2; }
    return x | (x << (h + 1 - s));
}
__device__ __forceinline__ unsigned long long jf_smear_down(unsigned long long x, int h) {
    int s = 1;
    while (2 * s <= h + 1) { x |= x >> s; s *= 2; }
    return x | (x >> (h + 1 - s));
}

// the word at wx of row `row` dilated horizontally by h, 0 <= h <= 40
__device__ __forceinline__ unsigned long long jf_hdilate(const unsigned long long* __restrict__ row, int wx, int WW, int h) {
    const unsigned long long C = row[wx];
    if (h == 0) return C;
    unsigned long long out = jf_smear_up(C, h) | jf_smear_down(C, h);
    if (wx > 0) {
        const unsigned long long tl = row[wx - 1] >> (64 - h);            // its top h columns; bit i lies h - i columns left of this word
        if (tl) out |= ~0ull >> __clzll((long long)tl);                   // ... and reaches columns 0 .. i: everything up to the highest i
    }
    if (wx + 1 < WW) {
        const unsigned long long tr = row[wx + 1] & ((1ull << h) - 1ull);  // its first h columns; bit i reaches columns 64 + i - h .. 63
        if (tr) out |= ~0ull << (64 - h + (__ffsll((long long)tr) - 1));
    }
    return out;
}

// launch 3: grid = (ceil(H * WW / 256), 2 n); blockIdx.y = 2 k + direction
__global__ __launch_bounds__(256) void jf_match_kernel(const unsigned long long* __restrict__ bnd, int H, int WW, int n, int r, JfSpans spans,
                                                       int* __restrict__ counts) {
    __shared__ int red[4];
    const int t = threadIdx.x;
    const int k = blockIdx.y >> 1, dir = blockIdx.y & 1;
    const long NW = (long)H * WW;
    const long g = (long)blockIdx.x * 256 + t;
    int matched = 0;
    if (g < NW) {
        const unsigned long long A = bnd[((long)dir * n + k) * NW + g];
        if (A) {
            const unsigned long long* B = bnd + ((long)(1 - dir) * n + k) * NW;
            const int y = (int)(g / WW), wx = (int)(g % WW);
            unsigned long long dil = jf_hdilate(B + (long)y * WW, wx, WW, spans.h[0]);
            for (int d = 1; d <= r && (A & ~dil); ++d) {
                const int h = spans.h[d];
                if (y - d >= 0) dil |= jf_hdilate(B + (long)(y - d) * WW, wx, WW, h);
                if (y + d < H) dil |= jf_hdilate(B + (long)(y + d) * WW, wx, WW, h);
            }
            matched = __popcll(A & dil);
        }
    }
    for (int off = 32; off > 0; off >>= 1) matched += __shfl_xor(matched, off, 64);
    if ((t & 63) == 0) red[t >> 6] = matched;
    __syncthreads();
    if (t == 0) {
        const int sum = red[0] + red[1] + red[2] + red[3];
        if (sum) atomicAdd(counts + k * 8 + 4 + dir, sum);
    }
}

// PROB_TO_ID flags == 64.  p2 = predicted ids u8 [H, W], p3 = ground-truth ids u8 [H, W], p6 = object ids int32 [i9], i5 = r,
// p7 = counts int32 [i9, 8], p5 = scratch int32 [i8]
int launch_jf_counts(const cutie_op* op, hipStream_t s) {
    const uint64_t* p = op->p;
    const int H = op->i[1], W = op->i[2], r = op->i[5], n = op->i[9];
    if (H < 1 || W < 1) { cutie_set_error("jf counts: empty shape (H, W >= 1)"); return -2; }
    if ((long)H * W >= (1l << 31)) { cutie_set_error("jf counts: %d x %d exceeds 2^31 pixels", H, W); return -2; }
    if (n < 1 || n > 255) { cutie_set_error("jf counts: %d objects, 1 <= n <= 255", n); return -2; }
    if (r < 1 || r > JF_MAX_RADIUS) { cutie_set_error("jf counts: radius %d, 1 <= r <= %d", r, JF_MAX_RADIUS); return -2; }
    if (!p[2] || !p[3] || !p[5] || !p[6] || !p[7]) {
        cutie_set_error("jf counts: needs the predicted ids (p2), the ground-truth ids (p3), the scratch (p5), the object ids (p6) and the counts (p7)");
        return -2;
    }
    if ((p[6] & 3) || (p[5] & 15) || (p[7] & 15)) {
        cutie_set_error("jf counts: object ids 4-byte aligned, scratch and counts 16-byte aligned");
        return -2;
    }
    const int WW = (W + 63) / 64;
    const long NW = (long)H * WW;
    const long need = 4l * n * NW;                            // two planes of n objects, two int32 words per 64 columns
    if ((long)op->i[8] < need) { cutie_set_error("jf counts: scratch of %d words, needs %ld", op->i[8], need); return -2; }
    JfSpans spans;
    for (int d = 0; d <= JF_MAX_RADIUS; ++d) {
        int h = 0;
        if (d <= r)
            while ((h + 1) * (h + 1) + d * d <= r * r) ++h;
        spans.h[d] = (unsigned char)h;
    }
    unsigned long long* bnd = (unsigned long long*)p[5];
    int* counts = (int*)p[7];
    const long per_block = 4 * JF_WORDS_PER_WAVE;
    hipLaunchKernelGGL(jf_zero_kernel, dim3((n * 8 + 255) / 256), dim3(256), 0, s, counts, n * 8);
    hipLaunchKernelGGL(jf_pack_kernel, dim3((unsigned)((NW + per_block - 1) / per_block)), dim3(256), 0, s, (const uint8_t*)p[2], (const uint8_t*)p[3], H, W, WW,
                       (const int*)p[6], n, bnd, counts);
    hipLaunchKernelGGL(jf_match_kernel, dim3((unsigned)((NW + 255) / 256), 2 * n), dim3(256), 0, s, (const unsigned long long*)bnd, H, WW, n, r, spans, counts);
    return (int)hipGetLastError();
}
