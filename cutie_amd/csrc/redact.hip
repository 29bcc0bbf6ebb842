// PROB_TO_ID flags == 65536 (ABI 11, form added): a frame with the tracked objects blurred, pixelated or painted over -- or, with the invert
// bit, everything but them.  frame uint8 [H, W, 3], weight plane uint8 [H, W] -> out uint8 [H, W, 3]: out = (w' e + (255 - w') f + 127) / 255
// with e the effect's byte.  Integers only; the contract is stated in include/cutie_hip.h and restated in tests/redact_ref.py; the bytes are
// equal.  ResultSaver(redact=...), process_video --redact, DESIGN.md section 26.
//
// BLUR      three launches of rd_box_kernel<LAST>: frame -> scratch A -> scratch B -> (blend) out.  One pass is a 2-D window mean rounded
//           once.  A block owns TX = RD_T - 2 r columns x TY rows of output and RD_T threads, one per pixel column of the tile with its
//           halo.  A thread keeps the VERTICAL window sums of its column's three channels in registers and slides them down the rows: one
//           row enters, one leaves (integers: sliding is exact).  Per row the HORIZONTAL window is the difference of two entries of a
//           block-wide prefix sum (wave scans by shuffles, the waves' totals through LDS).  A window sum is at most 255 * 129^2 < 2^23.
//           The third pass blends under the weight plane instead of storing the effect.
// PIXELATE  rd_cell_cols (per cell row and byte column the sum down the cell's rows, coalesced), rd_cell_mean (per cell and channel the
//           sum of its columns' sums in a fixed order, the rounded mean as a byte), rd_blend_kernel.
// FILL      rd_blend_kernel alone.
// No atomics, no grid barrier; every byte and word is written once by one thread and read behind a kernel boundary.  Every store is checked
// against its buffer.
#include "common.h"

#define RD_T 256               // threads per block of a blur pass: the columns of a tile, both halos included (OpList.REDACT_THREADS)
#define RD_RMAX 64             // the largest radius (OpList.REDACT_MAX_RADIUS, CUTIE_REDACT_MAX_RADIUS)
#define RD_CMAX 256            // the largest cell (OpList.REDACT_MAX_CELL)
#define RD_TY_SMALL 32         // output rows per block for r <= RD_R_SMALL (OpList.REDACT_TILE_Y)
#define RD_TY_LARGE 64         // ... for larger radii
#define RD_R_SMALL 16
#define RD_LD (RD_T + 1)       // a prefix row: entry 0 is zero

struct RdArgs {
    const uint8_t* src;        // [H, W, 3], row stride lds
    const uint8_t* frame;      // [H, W, 3], row stride ldf (the blend's f)
    const uint8_t* weight;     // [H, W], row stride ldw
    uint8_t* dst;              // [H, W, 3] contiguous
    size_t dst_bytes;
    int H, W, r, c, ldf, ldw, nbx, tx, ty, inv;
    long lds;
    uint32_t color;            // R | G << 8 | B << 16
    uint32_t* sums;            // pixelate: [CY][3 W] column sums
    size_t sums_words;
    uint8_t* cells;            // pixelate: [CY][CX][3] the cells' bytes
    size_t cells_bytes;
    int CY, CX;
};

__device__ __forceinline__ uint32_t rd_blend(uint32_t w, uint32_t e, uint32_t f) { return (w * e + (255u - w) * f + 127u) / 255u; }

// window sums over the columns t - r .. t + r of the block for three quantities: v is scanned in place, out is valid for r <= t < RD_T - r.
// Two barriers; the caller may call again at once (the next call's first barrier separates this call's reads from its writes).
__device__ __forceinline__ void rd_window(uint32_t (&v)[3], uint32_t* P, uint32_t* wt, int t, int r, uint32_t (&out)[3]) {
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        uint32_t x = v[q];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        v[q] = x;
        if (lane == 63) wt[q * 4 + wave] = x;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; q++) {
        uint32_t off = 0;
#pragma unroll
        for (int w = 0; w < 3; w++)
            if (w < wave) off += wt[q * 4 + w];
        P[q * RD_LD + t + 1] = v[q] + off;
    }
    __syncthreads();
    const int lo = max(t - r, 0), hi = min(t + r + 1, RD_T);
#pragma unroll
    for (int q = 0; q < 3; q++) out[q] = P[q * RD_LD + hi] - P[q * RD_LD + lo];
}

// row y of pixel column gx enters (SIGN = 1) or leaves (SIGN = -1, as an unsigned: modulo 2^32) the column's sums
template <int SIGN>
__device__ __forceinline__ void rd_row(const RdArgs& a, int y, int gx, uint32_t (&v)[3]) {
    const uint8_t* g = a.src + (size_t)y * a.lds + (size_t)gx * 3;
    const uint32_t sg = (uint32_t)SIGN;
    v[0] += sg * g[0]; v[1] += sg * g[1]; v[2] += sg * g[2];
}

// one box pass: dst = the rounded window mean of src (LAST = false), or the blend of it with the frame under the weight plane (LAST = true)
template <bool LAST>
__global__ __launch_bounds__(RD_T) void rd_box_kernel(RdArgs a) {
    __shared__ uint32_t P[3 * RD_LD];
    __shared__ uint32_t wt[3 * 4];
    const int t = threadIdx.x, r = a.r, H = a.H, W = a.W;
    const int bx = blockIdx.x % a.nbx, by = blockIdx.x / a.nbx;
    const int gx = bx * a.tx - r + t, y0 = by * a.ty, y1 = min(y0 + a.ty, H);
    const bool col = gx >= 0 && gx < W;                                  // a column of the frame (RD_T == tx + 2 r: every thread is in the tile)
    const bool outp = t >= r && t < r + a.tx && gx < W;
    if (t < 3) P[t * RD_LD] = 0;
    uint32_t v[3] = {0, 0, 0};
    if (col)
        for (int y = max(y0 - r, 0); y <= min(y0 + r, H - 1); y++) rd_row<1>(a, y, gx, v);
    const uint32_t nx = (uint32_t)(min(gx + r, W - 1) - max(gx - r, 0) + 1);
    for (int y = y0; y < y1; y++) {
        uint32_t sc[3] = {v[0], v[1], v[2]}, sw[3];
        rd_window(sc, P, wt, t, r, sw);
        if (outp) {
            const uint32_t N = (uint32_t)(min(y + r, H - 1) - max(y - r, 0) + 1) * nx;
            const size_t at = ((size_t)y * W + gx) * 3;
            uint32_t w = 0;
            const uint8_t* f = nullptr;
            if (LAST) {
                w = a.weight[(size_t)y * a.ldw + gx];
                if (a.inv) w = 255u - w;
                f = a.frame + (size_t)y * a.ldf + (size_t)gx * 3;
            }
#pragma unroll
            for (int q = 0; q < 3; q++) {
                uint32_t e = (2u * sw[q] + N) / (2u * N);
                if (LAST) e = rd_blend(w, e, f[q]);
                if (at + q < a.dst_bytes) a.dst[at + q] = (uint8_t)e;
            }
        }
        if (col && y + 1 < y1) {
            if (y + 1 + r <= H - 1) rd_row<1>(a, y + 1 + r, gx, v);
            if (y - r >= 0) rd_row<-1>(a, y - r, gx, v);
        }
    }
}

// pixelate 1: sums[Y][j] = the sum of byte column j (0 .. 3 W - 1) of the frame over the rows of cell row Y
__global__ __launch_bounds__(256) void rd_cell_cols(RdArgs a) {
    const size_t n3 = 3 * (size_t)a.W, id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (size_t)a.CY * n3) return;
    const int Y = (int)(id / n3);
    const size_t j = id % n3;
    const int ya = Y * a.c, yb = (int)min((long)a.H, (long)ya + a.c);
    uint32_t s = 0;
    for (int y = ya; y < yb; y++) s += a.frame[(size_t)y * a.ldf + j];
    if (id < a.sums_words) a.sums[id] = s;
}

// pixelate 2: cells[Y][X][ch] = (2 S + n) / (2 n) of cell (Y, X): its columns' sums added left to right
__global__ __launch_bounds__(256) void rd_cell_mean(RdArgs a) {
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (size_t)a.CY * a.CX * 3) return;
    const int ch = (int)(id % 3), X = (int)((id / 3) % a.CX), Y = (int)(id / 3 / a.CX);
    const int xa = X * a.c, xb = (int)min((long)a.W, (long)xa + a.c);
    const int rows = (int)min((long)a.H, (long)Y * a.c + a.c) - Y * a.c;
    const uint32_t* s = a.sums + (size_t)Y * 3 * a.W + ch;
    uint32_t S = 0;
    for (int x = xa; x < xb; x++) S += s[(size_t)x * 3];
    const uint32_t n = (uint32_t)rows * (uint32_t)(xb - xa);
    if (id < a.cells_bytes) a.cells[id] = (uint8_t)((2u * S + n) / (2u * n));
}

// the blend of a constant colour (CELLS = false) or of the cells' bytes (CELLS = true): a thread per pixel
template <bool CELLS>
__global__ __launch_bounds__(256) void rd_blend_kernel(RdArgs a) {
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (size_t)a.H * a.W) return;
    const int y = (int)(id / a.W), x = (int)(id % a.W);
    uint32_t w = a.weight[(size_t)y * a.ldw + x];
    if (a.inv) w = 255u - w;
    const uint8_t* f = a.frame + (size_t)y * a.ldf + (size_t)x * 3;
    const uint8_t* cell = CELLS ? a.cells + ((size_t)(y / a.c) * a.CX + x / a.c) * 3 : nullptr;
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const uint32_t e = CELLS ? cell[q] : (a.color >> (8 * q)) & 255u;
        if (id * 3 + q < a.dst_bytes) a.dst[id * 3 + q] = (uint8_t)rd_blend(w, e, f[q]);
    }
}

static bool rd_overlap(uint64_t a, uint64_t na, uint64_t b, uint64_t nb) { return a < b + nb && b < a + na; }

// int32 words of the scratch (OpList.redact_scratch_words): blur: two uint8 RGB images, each rounded up to a word; pixelate: the column
// sums [CY][3 W] and the cells' bytes; fill: one word that is never touched (the pointer is not null)
static uint64_t rd_scratch_words(int mode, int H, int W, int c) {
    if (mode == 0) return 2 * ((3ull * H * W + 3) / 4);
    if (mode == 1) {
        const uint64_t CY = ((uint64_t)H + c - 1) / c, CX = ((uint64_t)W + c - 1) / c;
        return CY * 3 * W + (CY * CX * 3 + 3) / 4;
    }
    return 1;
}

// PROB_TO_ID flags == 65536 (slots: include/cutie_hip.h).  p2 = frame u8 [H, W, 3] (i4 = row stride), p6 = weight u8 [H, W] (i5 = row stride),
// p3 = out u8 [H, W, 3], p5 = scratch int32 of i8 + 2^31 i7 words, i6 = mode, i3 = strength, i9 = invert, i10 = R | G << 8 | B << 16
int launch_redact(const cutie_op* op, hipStream_t s) {
    const uint64_t* p = op->p;
    const int* i = op->i;
    const int H = i[1], W = i[2], strength = i[3], ldf = i[4], ldw = i[5], mode = i[6], inv = i[9], color = i[10];
    if (H < 1 || W < 1 || (long)H * W >= (1l << 31)) { cutie_set_error("redact: H, W >= 1 and H * W < 2^31, not %d x %d", H, W); return -2; }
    if (mode < 0 || mode > 2) { cutie_set_error("redact: unknown mode %d (0 blur, 1 pixelate, 2 fill)", mode); return -2; }
    if (mode == 0 && (strength < 1 || strength > RD_RMAX)) { cutie_set_error("redact: blur radius %d, 1 .. %d", strength, RD_RMAX); return -2; }
    if (mode == 1 && (strength < 2 || strength > RD_CMAX)) { cutie_set_error("redact: pixelate cell %d, 2 .. %d", strength, RD_CMAX); return -2; }
    if (inv < 0 || inv > 1 || color < 0 || color > 0xffffff) { cutie_set_error("redact: the invert bit (i9 = %d) is 0 or 1 and the colour (i10 = %d) three bytes", inv, color); return -2; }
    if (!p[2] || !p[6] || !p[3] || !p[5]) { cutie_set_error("redact: needs the frame (p2), the weight plane (p6), the output (p3) and the scratch (p5)"); return -2; }
    if (ldf < 3 * W) { cutie_set_error("redact: frame row stride (i4 = %d) below a row's %d bytes", ldf, 3 * W); return -2; }
    if (ldw < W) { cutie_set_error("redact: weight row stride (i5 = %d) below a row's %d bytes", ldw, W); return -2; }
    if (p[5] & 3) { cutie_set_error("redact: scratch (p5) 4-byte aligned"); return -2; }
    if (i[7] < 0 || i[8] < 0) { cutie_set_error("redact: negative scratch size"); return -2; }
    const uint64_t words = (uint64_t)i[8] + ((uint64_t)i[7] << 31), need = rd_scratch_words(mode, H, W, strength), nout = 3ull * H * W;
    if (words < need) { cutie_set_error("redact: scratch of %llu words, needs %llu", (unsigned long long)words, (unsigned long long)need); return -2; }
    const uint64_t nframe = (uint64_t)(H - 1) * ldf + 3ull * W, nweight = (uint64_t)(H - 1) * ldw + W;
    if (rd_overlap(p[3], nout, p[2], nframe) || rd_overlap(p[3], nout, p[6], nweight) || rd_overlap(p[3], nout, p[5], need * 4) ||
        rd_overlap(p[5], need * 4, p[2], nframe) || rd_overlap(p[5], need * 4, p[6], nweight)) {
        cutie_set_error("redact: the output and the scratch overlap neither each other nor the frame or the weight plane");
        return -2;
    }
    RdArgs a = {};
    a.frame = (const uint8_t*)p[2]; a.weight = (const uint8_t*)p[6];
    a.H = H; a.W = W; a.ldf = ldf; a.ldw = ldw; a.inv = inv; a.color = (uint32_t)color;
    const unsigned npix = (unsigned)(((uint64_t)H * W + 255) / 256);
    if (mode == 0) {
        a.r = strength;
        a.tx = RD_T - 2 * strength;
        a.ty = strength <= RD_R_SMALL ? RD_TY_SMALL : RD_TY_LARGE;
        a.nbx = (W + a.tx - 1) / a.tx;
        const unsigned nblk = (unsigned)a.nbx * (unsigned)((H + a.ty - 1) / a.ty);
        uint8_t* A = (uint8_t*)p[5];
        uint8_t* B = A + 4 * (need / 2);
        a.src = a.frame; a.lds = ldf; a.dst = A; a.dst_bytes = (size_t)nout;
        hipLaunchKernelGGL(rd_box_kernel<false>, dim3(nblk), dim3(RD_T), 0, s, a);
        a.src = A; a.lds = 3l * W; a.dst = B;
        hipLaunchKernelGGL(rd_box_kernel<false>, dim3(nblk), dim3(RD_T), 0, s, a);
        a.src = B; a.dst = (uint8_t*)p[3];
        hipLaunchKernelGGL(rd_box_kernel<true>, dim3(nblk), dim3(RD_T), 0, s, a);
    } else if (mode == 1) {
        a.c = strength;
        a.CY = (H + strength - 1) / strength; a.CX = (W + strength - 1) / strength;
        a.sums = (uint32_t*)p[5]; a.sums_words = (size_t)a.CY * 3 * W;
        a.cells = (uint8_t*)(a.sums + a.sums_words); a.cells_bytes = (size_t)a.CY * a.CX * 3;
        a.dst = (uint8_t*)p[3]; a.dst_bytes = (size_t)nout;
        hipLaunchKernelGGL(rd_cell_cols, dim3((unsigned)((a.sums_words + 255) / 256)), dim3(256), 0, s, a);
        hipLaunchKernelGGL(rd_cell_mean, dim3((unsigned)((a.cells_bytes + 255) / 256)), dim3(256), 0, s, a);
        hipLaunchKernelGGL(rd_blend_kernel<true>, dim3(npix), dim3(256), 0, s, a);
    } else {
        a.dst = (uint8_t*)p[3]; a.dst_bytes = (size_t)nout;
        hipLaunchKernelGGL(rd_blend_kernel<false>, dim3(npix), dim3(256), 0, s, a);
    }
    return (int)hipGetLastError();
}
