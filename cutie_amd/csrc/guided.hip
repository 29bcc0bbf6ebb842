// PROB_TO_ID flags == 32768 (ABI 11, form added): the colour guided filter (He, Sun, Tang) of S uint8 planes under a packed uint8 RGB guide,
// the refinement of the alpha matte, the cut-out's fourth channel and the soft masks.  The contract -- integer window sums, a float64 solve
// per pixel in a written-out order, fixed-point coefficients, integer window sums again, a float64 evaluation -- is stated operation by
// operation in include/cutie_hip.h; tests/guided_ref.py is the same in numpy; the bytes are equal.  ResultSaver(matte_refine=(r, eps)),
// process_video --refine-matte, DESIGN.md section 25.
//
// Two launches with the coefficients in the scratch between them (a coefficient is read by (2r + 1)^2 neighbours: a grid-wide dependency):
//   1  gf_coef_kernel<SP>  a block owns GF_TX columns x GF_TY rows of output and GF_T = GF_TX + 2 * 64 threads, one per column of the tile
//                          with its halo.  A thread keeps the VERTICAL window sums of its column in registers -- 9 guide moments and 4 per
//                          plane, uint32 -- and slides them down the rows: one row enters, one leaves (the sums are integers: sliding is
//                          exact).  Per row the HORIZONTAL window is the difference of two entries of a block-wide prefix sum (wave scans by
//                          shuffles, the waves' totals and the prefix through LDS).  Prefixes may wrap modulo 2^32: a window sum is at most
//                          16641 * 65025 < 2^32, so the difference is exact.  The guide's covariance, its adjugate and determinant are made
//                          once per pixel; the planes follow in batches of GF_PB through the same LDS.  SP = S rounded up to 1, 2, 4, 8, 16
//                          keeps the planes' sums in registers (a runtime-indexed array would live in scratch memory).
//   2  gf_apply_kernel     the same tiling, one plane per blockIdx.y: int64 sums of the four coefficients, the evaluation, the byte.
// No atomics, no grid barrier; every word is written once by one thread and read behind the kernel boundary.  Every store is checked against
// its buffer.
#include "common.h"

#pragma clang fp contract(off)

#define GF_T 256               // threads per block: the columns of a tile, halo included (OpList.GUIDED_THREADS)
#define GF_RMAX 64             // the largest radius (OpList.GUIDED_MAX_RADIUS)
#define GF_TX (GF_T - 2 * GF_RMAX)     // 128 output columns per block (OpList.GUIDED_TILE_X)
#define GF_TY 64               // output rows per block (OpList.GUIDED_TILE_Y)
#define GF_MAXS 16             // planes per op (OpList.GUIDED_MAX_PLANES)
#define GF_PB 4                // planes per prefix-sum batch of launch 1
#define GF_LD (GF_T + 1)       // a prefix row: entry 0 is zero

struct GfArgs {
    const uint8_t* guide;      // [H, W, 3], row stride ldg
    const uint8_t* planes;     // [S0, H, W], row stride ldp, plane stride ps
    const uint8_t* last;       // optional plane S0, row stride ldl
    int H, W, r, S, S0, ldg, ldp, ldl, nbx;
    long ps;
    double eps;
    int32_t* coef;             // [S][4][H][W]
    size_t coef_words;
    uint8_t* out;              // [S][H][W]
    size_t out_bytes;
};

// window sums over the columns t - r .. t + r of the block for NQ quantities: v is scanned in place, out is valid for r <= t < GF_T - r.
// Two barriers; the caller may call again at once (the next call's first barrier separates this call's reads from its writes).
template <typename T, int NQ>
__device__ __forceinline__ void gf_window(T (&v)[NQ], T* P, T* wt, int t, int r, T (&out)[NQ]) {
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        T x = v[q];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const T y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        v[q] = x;
        if (lane == 63) wt[q * 4 + wave] = x;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        T off = 0;
#pragma unroll
        for (int w = 0; w < 3; w++)
            if (w < wave) off += wt[q * 4 + w];
        P[q * GF_LD + t + 1] = v[q] + off;
    }
    __syncthreads();
    const int lo = max(t - r, 0), hi = min(t + r + 1, GF_T);
#pragma unroll
    for (int q = 0; q < NQ; q++) out[q] = P[q * GF_LD + hi] - P[q * GF_LD + lo];
}

__device__ __forceinline__ const uint8_t* gf_plane(const GfArgs& a, int s) {
    return s < a.S0 ? a.planes + (size_t)s * a.ps : a.last;
}

__device__ __forceinline__ int gf_plane_ld(const GfArgs& a, int s) { return s < a.S0 ? a.ldp : a.ldl; }

// row y of column gx enters (SIGN = 1) or leaves (SIGN = -1, as an unsigned: modulo 2^32) the column's sums
template <int SP, int SIGN>
__device__ __forceinline__ void gf_row(const GfArgs& a, int y, int gx, uint32_t (&vg)[9], uint32_t (&vp)[SP][4]) {
    const uint8_t* g = a.guide + (size_t)y * a.ldg + (size_t)gx * 3;
    const uint32_t sg = (uint32_t)SIGN;
    const uint32_t i0 = g[0], i1 = g[1], i2 = g[2];
    vg[0] += sg * i0; vg[1] += sg * i1; vg[2] += sg * i2;
    vg[3] += sg * (i0 * i0); vg[4] += sg * (i0 * i1); vg[5] += sg * (i0 * i2);
    vg[6] += sg * (i1 * i1); vg[7] += sg * (i1 * i2); vg[8] += sg * (i2 * i2);
#pragma unroll
    for (int s = 0; s < SP; s++) {
        if (s < a.S) {
            const uint32_t p = gf_plane(a, s)[(size_t)y * gf_plane_ld(a, s) + gx];
            vp[s][0] += sg * p; vp[s][1] += sg * (i0 * p); vp[s][2] += sg * (i1 * p); vp[s][3] += sg * (i2 * p);
        }
    }
}

__device__ __forceinline__ int gf_sat(double x) {           // sat_int32(rint(x)), round-half-even
    return (int)fmin(fmax(rint(x), -2147483648.0), 2147483647.0);
}

template <int SP>
__global__ __launch_bounds__(GF_T) void gf_coef_kernel(GfArgs a) {
    __shared__ uint32_t P[4 * GF_PB * GF_LD];
    __shared__ uint32_t wt[4 * GF_PB * 4];
    const int t = threadIdx.x, r = a.r, H = a.H, W = a.W;
    const int bx = blockIdx.x % a.nbx, by = blockIdx.x / a.nbx;
    const int gx = bx * GF_TX - r + t, y0 = by * GF_TY, y1 = min(y0 + GF_TY, H);
    const bool col = gx >= 0 && gx < W && t < GF_TX + 2 * r;            // a column of the frame that some output of this block reads
    const bool outp = t >= r && t < r + GF_TX && gx < W;
    if (t < 4 * GF_PB) P[t * GF_LD] = 0;
    uint32_t vg[9], vp[SP][4];
#pragma unroll
    for (int q = 0; q < 9; q++) vg[q] = 0;
#pragma unroll
    for (int s = 0; s < SP; s++) { vp[s][0] = vp[s][1] = vp[s][2] = vp[s][3] = 0; }
    if (col)
        for (int y = max(y0 - r, 0); y <= min(y0 + r, H - 1); y++) gf_row<SP, 1>(a, y, gx, vg, vp);
    const int nx = min(gx + r, W - 1) - max(gx - r, 0) + 1;
    for (int y = y0; y < y1; y++) {
        uint32_t sc[9], sw[9];
#pragma unroll
        for (int q = 0; q < 9; q++) sc[q] = vg[q];
        gf_window<uint32_t, 9>(sc, P, wt, t, r, sw);
        const long N = (long)(min(y + r, H - 1) - max(y - r, 0) + 1) * nx;
        double a00, a01, a02, a11, a12, a22, det;
        const long S0 = sw[0], S1 = sw[1], S2 = sw[2];
        if (outp) {
            // stage 1: C = N S_cd - S_c S_d in int64; stage 2: M = C + e Id, e = ((eps 65025) N) N, the symmetric adjugate, the determinant
            const double e = ((a.eps * 65025.0) * (double)N) * (double)N;
            const double m00 = (double)(N * (long)sw[3] - S0 * S0) + e, m01 = (double)(N * (long)sw[4] - S0 * S1), m02 = (double)(N * (long)sw[5] - S0 * S2);
            const double m11 = (double)(N * (long)sw[6] - S1 * S1) + e, m12 = (double)(N * (long)sw[7] - S1 * S2);
            const double m22 = (double)(N * (long)sw[8] - S2 * S2) + e;
            a00 = m11 * m22 - m12 * m12;
            a01 = m02 * m12 - m01 * m22;
            a02 = m01 * m12 - m02 * m11;
            a11 = m00 * m22 - m02 * m02;
            a12 = m01 * m02 - m00 * m12;
            a22 = m00 * m11 - m01 * m01;
            det = (m00 * a00 + m01 * a01) + m02 * a02;
        }
#pragma unroll
        for (int b = 0; b < SP; b += GF_PB) {
            constexpr int NB = SP < GF_PB ? SP : GF_PB;
            uint32_t pc[4 * NB], pw[4 * NB];
#pragma unroll
            for (int k = 0; k < NB; k++) { pc[4 * k] = vp[b + k][0]; pc[4 * k + 1] = vp[b + k][1]; pc[4 * k + 2] = vp[b + k][2]; pc[4 * k + 3] = vp[b + k][3]; }
            if (b < a.S) gf_window<uint32_t, 4 * NB>(pc, P, wt, t, r, pw);     // (block-uniform)
            if (outp) {
#pragma unroll
                for (int k = 0; k < NB; k++) {
                    const int s = b + k;
                    if (s < a.S) {
                        const long T = pw[4 * k];
                        const double g0 = (double)(N * (long)pw[4 * k + 1] - S0 * T), g1 = (double)(N * (long)pw[4 * k + 2] - S1 * T),
                                     g2 = (double)(N * (long)pw[4 * k + 3] - S2 * T);
                        const double c0 = ((a00 * g0 + a01 * g1) + a02 * g2) / det;
                        const double c1 = ((a01 * g0 + a11 * g1) + a12 * g2) / det;
                        const double c2 = ((a02 * g0 + a12 * g1) + a22 * g2) / det;
                        const double bb = ((double)T - ((c0 * (double)S0 + c1 * (double)S1) + c2 * (double)S2)) / (double)N;
                        const int cf[4] = {gf_sat(c0 * 1048576.0), gf_sat(c1 * 1048576.0), gf_sat(c2 * 1048576.0), gf_sat(bb * 4096.0)};
#pragma unroll
                        for (int k4 = 0; k4 < 4; k4++) {
                            const size_t at = ((size_t)(s * 4 + k4) * H + y) * W + gx;
                            if (at < a.coef_words) a.coef[at] = cf[k4];
                        }
                    }
                }
            }
        }
        if (col && y + 1 < y1) {
            if (y + 1 + r <= H - 1) gf_row<SP, 1>(a, y + 1 + r, gx, vg, vp);
            if (y - r >= 0) gf_row<SP, -1>(a, y - r, gx, vg, vp);
        }
    }
}

template <int SIGN>
__device__ __forceinline__ void gf_coef_row(const int32_t* c, size_t plane, size_t at, long long (&v)[4]) {
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] += (long long)SIGN * c[k * plane + at];
}

__global__ __launch_bounds__(GF_T) void gf_apply_kernel(GfArgs a) {
    __shared__ long long P[4 * GF_LD];
    __shared__ long long wt[4 * 4];
    const int t = threadIdx.x, r = a.r, H = a.H, W = a.W, s = blockIdx.y;
    const int bx = blockIdx.x % a.nbx, by = blockIdx.x / a.nbx;
    const int gx = bx * GF_TX - r + t, y0 = by * GF_TY, y1 = min(y0 + GF_TY, H);
    const bool col = gx >= 0 && gx < W && t < GF_TX + 2 * r;
    const bool outp = t >= r && t < r + GF_TX && gx < W;
    if (t < 4) P[t * GF_LD] = 0;
    const size_t plane = (size_t)H * W;
    const int32_t* c = a.coef + (size_t)s * 4 * plane;
    long long v[4] = {0, 0, 0, 0};
    if (col)
        for (int y = max(y0 - r, 0); y <= min(y0 + r, H - 1); y++) gf_coef_row<1>(c, plane, (size_t)y * W + gx, v);
    const int nx = min(gx + r, W - 1) - max(gx - r, 0) + 1;
    for (int y = y0; y < y1; y++) {
        long long sc[4] = {v[0], v[1], v[2], v[3]}, sw[4];
        gf_window<long long, 4>(sc, P, wt, t, r, sw);
        if (outp) {
            const long N = (long)(min(y + r, H - 1) - max(y - r, 0) + 1) * nx;
            const uint8_t* g = a.guide + (size_t)y * a.ldg + (size_t)gx * 3;
            // stage 4: q = ((((sum A0) I0 + (sum A1) I1) + (sum A2) I2) 2^-20 + (sum B) 2^-12) / N
            const double q = ((((double)sw[0] * (double)g[0] + (double)sw[1] * (double)g[1]) + (double)sw[2] * (double)g[2]) * (1.0 / 1048576.0) +
                              (double)sw[3] * (1.0 / 4096.0)) / (double)N;
            const size_t at = (size_t)s * plane + (size_t)y * W + gx;
            if (at < a.out_bytes) a.out[at] = (uint8_t)fmin(fmax(rint(q), 0.0), 255.0);
        }
        if (col && y + 1 < y1) {
            if (y + 1 + r <= H - 1) gf_coef_row<1>(c, plane, (size_t)(y + 1 + r) * W + gx, v);
            if (y - r >= 0) gf_coef_row<-1>(c, plane, (size_t)(y - r) * W + gx, v);
        }
    }
}

static bool gf_overlap(uint64_t a, uint64_t na, uint64_t b, uint64_t nb) { return a < b + nb && b < a + na; }

// PROB_TO_ID flags == 32768 (slots: include/cutie_hip.h).  p2 = guide u8 [H, W, 3] (i4 = row stride), p6 = planes u8 [S0, H, W] (i5 = row
// stride, i6 = plane stride), p7 = optional last plane u8 [H, W] (i10 = row stride), i9 = S0, p3 = out u8 [S, H, W], p5 = scratch int32 of
// i8 + 2^31 i7 words, i3 = r, f0 = eps
int launch_guided_filter(const cutie_op* op, hipStream_t s) {
    const uint64_t* p = op->p;
    const int* i = op->i;
    const int H = i[1], W = i[2], r = i[3], ldg = i[4], ldp = i[5], ps = i[6], S0 = i[9], ldl = i[10];
    const float eps = op->f[0];
    if (H < 1 || W < 1 || (long)H * W >= (1l << 31)) { cutie_set_error("guided filter: H, W >= 1 and H * W < 2^31, not %d x %d", H, W); return -2; }
    if (r < 1 || r > GF_RMAX) { cutie_set_error("guided filter: radius %d, 1 .. %d", r, GF_RMAX); return -2; }
    if (!(eps >= 1e-6f && eps <= 1.0f)) { cutie_set_error("guided filter: eps %g, 1e-6 .. 1", (double)eps); return -2; }
    const int S = S0 + (p[7] ? 1 : 0);
    if (S0 < 0 || S < 1 || S > GF_MAXS) { cutie_set_error("guided filter: %d planes, 1 .. %d", S0 < 0 ? S0 : S, GF_MAXS); return -2; }
    if (!p[2] || !p[3] || !p[5] || (S0 > 0 && !p[6])) { cutie_set_error("guided filter: needs the guide (p2), the planes (p6 with i9 > 0), the output (p3) and the scratch (p5)"); return -2; }
    if (ldg < 3 * W) { cutie_set_error("guided filter: guide row stride (i4 = %d) below a row's %d bytes", ldg, 3 * W); return -2; }
    const long span = (long)(H - 1) * ldp + W;
    if ((S0 > 0 && (ldp < W || (S0 > 1 && ps < span))) || (p[7] && ldl < W)) {
        cutie_set_error("guided filter: plane strides (row i5 = %d, plane i6 = %d, last row i10 = %d) below a row's %d or a plane's %ld bytes", ldp, ps, ldl, W, span);
        return -2;
    }
    if (p[5] & 3) { cutie_set_error("guided filter: scratch (p5) 4-byte aligned"); return -2; }
    if (i[7] < 0 || i[8] < 0) { cutie_set_error("guided filter: negative scratch size"); return -2; }
    const uint64_t words = (uint64_t)i[8] + ((uint64_t)i[7] << 31), need = 4ull * S * H * W, nout = (uint64_t)S * H * W;
    if (words < need) { cutie_set_error("guided filter: scratch of %llu words, needs %llu", (unsigned long long)words, (unsigned long long)need); return -2; }
    const uint64_t nguide = (uint64_t)(H - 1) * ldg + 3ull * W, nplanes = S0 > 0 ? (uint64_t)(S0 - 1) * ps + span : 0, nlast = p[7] ? (uint64_t)(H - 1) * ldl + W : 0;
    if (gf_overlap(p[3], nout, p[2], nguide) || (nplanes && gf_overlap(p[3], nout, p[6], nplanes)) || (nlast && gf_overlap(p[3], nout, p[7], nlast)) ||
        gf_overlap(p[3], nout, p[5], need * 4) || gf_overlap(p[5], need * 4, p[2], nguide) || (nplanes && gf_overlap(p[5], need * 4, p[6], nplanes)) ||
        (nlast && gf_overlap(p[5], need * 4, p[7], nlast))) {
        cutie_set_error("guided filter: the output and the scratch overlap neither each other nor the guide or the planes");
        return -2;
    }
    GfArgs a;
    a.guide = (const uint8_t*)p[2]; a.planes = (const uint8_t*)p[6]; a.last = (const uint8_t*)p[7];
    a.H = H; a.W = W; a.r = r; a.S = S; a.S0 = S0; a.ldg = ldg; a.ldp = ldp; a.ldl = ldl; a.ps = ps;
    a.nbx = (W + GF_TX - 1) / GF_TX;
    a.eps = (double)eps;
    a.coef = (int32_t*)p[5]; a.coef_words = (size_t)need;
    a.out = (uint8_t*)p[3]; a.out_bytes = (size_t)nout;
    const unsigned nblk = (unsigned)a.nbx * (unsigned)((H + GF_TY - 1) / GF_TY);
    if (S == 1) hipLaunchKernelGGL(gf_coef_kernel<1>, dim3(nblk), dim3(GF_T), 0, s, a);
    else if (S == 2) hipLaunchKernelGGL(gf_coef_kernel<2>, dim3(nblk), dim3(GF_T), 0, s, a);
    else if (S <= 4) hipLaunchKernelGGL(gf_coef_kernel<4>, dim3(nblk), dim3(GF_T), 0, s, a);
    else if (S <= 8) hipLaunchKernelGGL(gf_coef_kernel<8>, dim3(nblk), dim3(GF_T), 0, s, a);
    else hipLaunchKernelGGL(gf_coef_kernel<16>, dim3(nblk), dim3(GF_T), 0, s, a);
    hipLaunchKernelGGL(gf_apply_kernel, dim3(nblk, S), dim3(GF_T), 0, s, a);
    return (int)hipGetLastError();
}
