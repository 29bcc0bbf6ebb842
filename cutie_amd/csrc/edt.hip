// PROB_TO_ID flags == 4096 (ABI 11, form added): the exact squared Euclidean distance transform of a uint8 id plane [H, W] for S sets of
// ids, and the band byte that erosion, dilation and trimaps of any radius are a compare of (slots and conventions: include/cutie_hip.h;
// the numpy model: tests/edt_ref.py).
//
// Per set a pixel is of class 1 (its id is in the set) or 0.  D(p) = min(limit, the smallest dx^2 + dy^2 to a pixel of the OTHER class
// inside the frame).  The transform is separable for two classes: with g(x, y) = the vertical distance from (x, y) to the nearest pixel
// of the other class THAN (x, y) ITSELF in column x, a pixel (x, y) of class c finds in column x + dx
//   dx^2                        where (x + dx, y) is of the other class (nothing in that column is nearer than its own row), and
//   dx^2 + g(x + dx, y)^2       where (x + dx, y) is of class c (g is measured from a pixel of c: it is the column's nearest of the other).
// Two launches over one uint16 per (set, pixel) in the scratch, class in bit 15, g in the low bits:
//   1  edt_col_kernel   one thread per (column, chunk of rows, set); the plane's bytes are read coalesced across x.  g is capped at R = the
//                       smallest r with r^2 >= limit (the cap also says "none in this column": dx^2 + R^2 >= limit never lowers D), so a
//                       walk that starts R - 1 rows above the chunk knows everything the chunk's rows can see: the thread walks down
//                       from there, stores the chunk's rows, walks up from R - 1 rows below the chunk and stores the minimum.  It writes
//                       no word but its own chunk's and reads none but those.  Chunks are max(EDT_CH, R) rows: at most 3 x the work
//                       of one walk per column, and H / chunk times the threads.
//   2  edt_row_kernel   one block per (segment of EDT_T pixels, row, set): the row's words of the segment and R - 1 columns on each side
//                       go into LDS; a thread scans dx = 0, 1, 2 ... on both sides and stops when dx^2 reaches its running minimum
//                       (<= limit, so dx <= R - 1: the halo).  It writes D, the band byte, or both.
// Everything is integer; every word is written once, by one thread, and read behind a kernel boundary: no atomics, nothing depends on
// launch shape or arrival order.
#include "common.h"

#define EDT_CW 64                        // columns per block of launch 1: OpList.EDT_COL_GROUP
#define EDT_CH 32                        // least rows per chunk of launch 1: OpList.EDT_ROW_CHUNK
#define EDT_T 256                        // pixels per row segment of launch 2: OpList.EDT_ROW_SEGMENT
#define EDT_RMAX 256                     // R at CUTIE_EDT_MAX_LIMIT
#define EDT_CLASS 0x8000u

__global__ __launch_bounds__(EDT_CW) void edt_col_kernel(const uint8_t* __restrict__ ids, const uint8_t* __restrict__ sets, int H, int W, int R, int CH,
                                                         int ncg, int nch, uint16_t* __restrict__ g) {
    __shared__ uint8_t s_in[256];
    const unsigned b = blockIdx.x;
    const int cg = (int)(b % (unsigned)ncg), ch = (int)((b / (unsigned)ncg) % (unsigned)nch), s = (int)(b / ((unsigned)ncg * (unsigned)nch));
    for (int k = threadIdx.x; k < 256; k += EDT_CW) s_in[k] = sets[s * 256 + k] != 0;
    __syncthreads();
    const int x = cg * EDT_CW + (int)threadIdx.x;
    if (x >= W) return;
    const int y0 = ch * CH, y1 = min(H, y0 + CH);
    const uint8_t* col = ids + x;
    uint16_t* out = g + (long)s * H * W + x;
    int d = R, prev = -1;
    for (int y = max(0, y0 - (R - 1)); y < y1; ++y) {          // down: the nearest pixel of the other class above
        const int c = s_in[col[(long)y * W]];
        d = (prev >= 0 && c != prev) ? 1 : min(d + 1, R);
        prev = c;
        if (y >= y0) out[(long)y * W] = (uint16_t)((unsigned)d | (c ? EDT_CLASS : 0u));
    }
    d = R, prev = -1;
    for (int y = min(H - 1, y1 - 1 + (R - 1)); y >= y0; --y) { // up: the nearest one below; the minimum of both
        const int c = s_in[col[(long)y * W]];
        d = (prev >= 0 && c != prev) ? 1 : min(d + 1, R);
        prev = c;
        if (y < y1) {
            const unsigned down = out[(long)y * W] & ~EDT_CLASS;           // (this thread's own store)
            out[(long)y * W] = (uint16_t)(min((unsigned)d, down) | (c ? EDT_CLASS : 0u));
        }
    }
}

__global__ __launch_bounds__(EDT_T) void edt_row_kernel(const uint16_t* __restrict__ g, int H, int W, int R, int nseg, int inner, int outer, int limit,
                                                        int mid, int* __restrict__ dist2, uint8_t* __restrict__ band) {
    __shared__ uint16_t s_g[EDT_T + 2 * (EDT_RMAX - 1)];
    const unsigned b = blockIdx.x;
    const int seg = (int)(b % (unsigned)nseg), y = (int)((b / (unsigned)nseg) % (unsigned)H), s = (int)(b / ((unsigned)nseg * (unsigned)H));
    const int halo = R - 1, x0 = seg * EDT_T, lo = max(0, x0 - halo), hi = min(W, x0 + EDT_T + halo);      // columns [lo, hi) of the row
    const long row = ((long)s * H + y) * W;
    for (int k = lo + (int)threadIdx.x; k < hi; k += EDT_T) s_g[k - lo] = g[row + k];
    __syncthreads();
    const int x = x0 + (int)threadIdx.x;
    if (x >= W) return;
    const unsigned own = s_g[x - lo], c = own & EDT_CLASS;
    const int g0 = (int)(own & ~EDT_CLASS);
    int best = min(limit, g0 * g0);
    for (int dx = 1; dx * dx < best; ++dx) {                   // (best <= limit <= R^2: dx <= R - 1, inside [lo, hi) where inside the frame)
        const int d2 = dx * dx;
        if (x - dx >= 0) {
            const unsigned v = s_g[x - dx - lo];
            const int gv = (int)(v & ~EDT_CLASS);
            best = min(best, (v & EDT_CLASS) != c ? d2 : d2 + gv * gv);
        }
        if (x + dx < W) {
            const unsigned v = s_g[x + dx - lo];
            const int gv = (int)(v & ~EDT_CLASS);
            best = min(best, (v & EDT_CLASS) != c ? d2 : d2 + gv * gv);
        }
    }
    if (dist2) dist2[row + x] = best;
    if (band) band[row + x] = (uint8_t)(c ? (best > inner ? 255 : mid) : (best <= outer ? mid : 0));
}

// PROB_TO_ID flags == 4096.  p2 = ids u8 [i1, i2], read only; p6 = sets u8 [i9, 256]; i3 = inner, i4 = outer, i5 = limit, i6 = mid;
// p5 = scratch int32 [i8 + 2^31 i7]; p3 = band u8 [i9, i1, i2] or null; p7 = dist2 int32 [i9, i1, i2] or null
int launch_edt_band(const cutie_op* op, hipStream_t s) {
    const uint64_t* p = op->p;
    const int H = op->i[1], W = op->i[2], inner = op->i[3], outer = op->i[4], limit = op->i[5], mid = op->i[6], S = op->i[9];
    if (H < 1 || W < 1) { cutie_set_error("edt band: empty shape (H, W >= 1)"); return -2; }
    if ((long)H * W >= (1l << 31)) { cutie_set_error("edt band: %d x %d exceeds 2^31 pixels", H, W); return -2; }
    if (S < 1 || S > CUTIE_EDT_MAX_SETS) { cutie_set_error("edt band: %d sets, 1 <= S <= %d", S, CUTIE_EDT_MAX_SETS); return -2; }
    if (inner < 0 || outer < 0) { cutie_set_error("edt band: negative threshold (inner %d, outer %d)", inner, outer); return -2; }
    if (limit > CUTIE_EDT_MAX_LIMIT || limit <= (inner > outer ? inner : outer)) {
        cutie_set_error("edt band: limit %d, max(inner, outer) = %d < limit <= %d", limit, inner > outer ? inner : outer, CUTIE_EDT_MAX_LIMIT);
        return -2;
    }
    if (mid < 0 || mid > 255) { cutie_set_error("edt band: mid %d is a byte", mid); return -2; }
    if (!p[2]) { cutie_set_error("edt band: needs the id plane (p2)"); return -2; }
    if (!p[6]) { cutie_set_error("edt band: needs the sets (p6)"); return -2; }
    if (!p[5]) { cutie_set_error("edt band: needs the scratch (p5)"); return -2; }
    if (!p[3] && !p[7]) { cutie_set_error("edt band: needs band (p3), dist2 (p7) or both"); return -2; }
    if ((p[5] & 3) || (p[7] & 3)) { cutie_set_error("edt band: scratch and dist2 4-byte aligned"); return -2; }
    const long need = ((long)S * H * W + 1) / 2;
    const long words = (op->i[8] < 0 || op->i[7] < 0) ? -1l : (long)op->i[8] + ((long)op->i[7] << 31);
    if (words < need) { cutie_set_error("edt band: scratch of %ld words, %d sets of %d x %d need %ld", words, S, H, W, need); return -2; }
    int R = 1;
    while (R * R < limit) ++R;                                 // <= EDT_RMAX
    const int CH = R > EDT_CH ? R : EDT_CH;
    const int ncg = (W + EDT_CW - 1) / EDT_CW, nch = (H + CH - 1) / CH, nseg = (W + EDT_T - 1) / EDT_T;
    const long colb = (long)ncg * nch * S, rowb = (long)nseg * H * S;
    if (colb >= (1l << 31) || rowb >= (1l << 31)) { cutie_set_error("edt band: %d sets of %d x %d exceed 2^31 blocks", S, H, W); return -2; }
    uint16_t* g = (uint16_t*)p[5];
    hipLaunchKernelGGL(edt_col_kernel, dim3((unsigned)colb), dim3(EDT_CW), 0, s, (const uint8_t*)p[2], (const uint8_t*)p[6], H, W, R, CH, ncg, nch, g);
    hipLaunchKernelGGL(edt_row_kernel, dim3((unsigned)rowb), dim3(EDT_T), 0, s, (const uint16_t*)g, H, W, R, nseg, inner, outer, limit, mid,
                       (int*)p[7], (uint8_t*)p[3]);
    return (int)hipGetLastError();
}
