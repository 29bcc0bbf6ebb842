// PROB_TO_ID flags == 256 / 512 (ABI 11, forms added): the visualisation modes, the alpha matte and the soft masks of the reference's interactive tool
// (gui/interactive_utils.py:79-229, gui/resource_manager.py:154-173), composed on the device from what a step leaves there: the
// probability planes, the uint8 frame and the id plane (ResultSaver vis_modes / soft_masks / alpha_matte,
// cutie_amd/inference/utils/results_utils.py).  The arithmetic -- float32, every multiply and add rounded on its own (the library is built
// with -ffp-contract=off), the operation order of the reference's torch expressions -- is listed in include/cutie_hip.h;
// tests/matte_ref.py is the same in numpy, the bytes are equal.
//
//   matte_composite_kernel   flags == 256: one mode -> a packed uint8 frame [OH, OW, 3] and / or the matte plane [OH, OW]
//   matte_soft_kernel        flags == 512: the P - 1 object planes quantised to uint8 [P - 1, OH, OW]
//
// Both are streaming passes without LDS.  A thread owns FOUR CONSECUTIVE PIXELS OF THE FLATTENED OUTPUT (n = 4 t .. 4 t + 3), so that its
// 12 bytes of RGB, its 4 ids / matte bytes and its 16 bytes of layer are whole, aligned dwords whatever OW is (854 is no multiple of 4);
// the lanes of a wave lie on consecutive groups.  The vertical taps and lambda are computed once per thread and shared by its pixels and
// by all planes; only a group that straddles the end of a row computes them per pixel.  The last group of an image whose pixel count is
// no multiple of 4, and inputs that are not flat and aligned (a padded or odd frame row stride), go byte by byte: the same bytes.
// A plane sample is resize_kernel's (= PROB_TO_ID flags&4) expression, operation for operation.
#include "common.h"

#define MATTE_DAVIS 0
#define MATTE_LIGHT 1
#define MATTE_FADE 2
#define MATTE_POPUP 3
#define MATTE_LAYER 4
#define MATTE_ALPHA 5                   // the matte plane alone
#define MATTE_MAX_TARGETS 255

struct MatteGeom {
    int P, H, W, OH, OW, ldrow;         // planes as stored: P x [H, W], row stride ldrow; output OH x OW
    long plane;                         // plane stride (elements)
    int resample;                       // (H, W) != (OH, OW)
    int pflat;                          // the planes are read with float4: same size, rows contiguous, plane stride and base 16-byte multiples
};
struct MatteTargets {
    int n;
    uint8_t q[256];                     // plane indices, in the order they are summed
};

// the four pixels of a thread: row, column and the taps of the plane sample
struct MattePix {
    int oy[4], ox[4];
    int y0[4], y1[4], x0[4], x1[4];
    float ly[4], lx[4];
};

__device__ __forceinline__ void matte_pixels(const MatteGeom& G, long n0, long N, MattePix& t) {
    int oy = (int)(n0 / G.OW), ox = (int)(n0 - (long)oy * G.OW);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (n0 + k >= N) { oy = G.OH - 1; ox = G.OW - 1; }          // (a pixel past the image repeats the last one; it is not stored)
        t.oy[k] = oy; t.ox[k] = ox;
        if (++ox >= G.OW) { ox = 0; ++oy; }
    }
    if (!G.resample) return;
    const float sy = (float)G.H / (float)G.OH, sx = (float)G.W / (float)G.OW;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k == 0 || t.oy[k] != t.oy[0]) {
            const float fy = fmaxf((t.oy[k] + 0.5f) * sy - 0.5f, 0.f);
            t.y0[k] = min((int)fy, G.H - 1);
            t.y1[k] = min(t.y0[k] + 1, G.H - 1);
            t.ly[k] = fy - (float)t.y0[k];
        } else { t.y0[k] = t.y0[0]; t.y1[k] = t.y1[0]; t.ly[k] = t.ly[0]; }
        const float fx = fmaxf((t.ox[k] + 0.5f) * sx - 0.5f, 0.f);
        t.x0[k] = min((int)fx, G.W - 1);
        t.x1[k] = min(t.x0[k] + 1, G.W - 1);
        t.lx[k] = fx - (float)t.x0[k];
    }
}

// plane q at the thread's four pixels
__device__ __forceinline__ void matte_plane(const float* __restrict__ planes, const MatteGeom& G, const MattePix& t, int q, long n0, bool full, float* v) {
    const float* p = planes + (long)q * G.plane;
    if (!G.resample) {
        if (G.pflat && full) {
            const float4 f = *(const float4*)(p + n0);
            v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
            return;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = p[(long)t.oy[k] * G.ldrow + t.ox[k]];
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float* r0 = p + (long)t.y0[k] * G.ldrow;
        const float* r1 = p + (long)t.y1[k] * G.ldrow;
        const float a = r0[t.x0[k]], b = r0[t.x1[k]], cc = r1[t.x0[k]], d = r1[t.x1[k]];
        const float ly = t.ly[k], lx = t.lx[k];
        v[k] = (1.f - ly) * ((1.f - lx) * a + lx * b) + ly * ((1.f - lx) * cc + lx * d);
    }
}

// (uint8)(x * 255.0f), the product clamped to [0, 255] (NaN -> 0)
__device__ __forceinline__ uint32_t matte_q8(float x) {
    const float q = fminf(fmaxf(x * 255.0f, 0.f), 255.f);
    return (uint32_t)(int)q;
}
__device__ __forceinline__ float matte_u8f(uint32_t b) { return (float)b / 255.0f; }     // correctly rounded: HIP's default fp32 '/'

extern "C" __global__ __launch_bounds__(256) void matte_composite_kernel(const float* __restrict__ planes, MatteGeom G, MatteTargets T,
                                                                         const uint8_t* __restrict__ frame, long ldf, int fflat,
                                                                         const uint8_t* __restrict__ ids, const uint32_t* __restrict__ ctab,
                                                                         const uint8_t* __restrict__ layer, uint8_t* __restrict__ out,
                                                                         uint8_t* __restrict__ matte, int mode, float ca, float cb) {
    const long N = (long)G.OH * G.OW, n0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (n0 >= N) return;
    const bool full = n0 + 4 <= N;
    MattePix t;
    matte_pixels(G, n0, N, t);

    float m[4] = {0.f, 0.f, 0.f, 0.f};
    if (mode >= MATTE_POPUP) {
        for (int j = 0; j < T.n; ++j) {
            float v[4];
            matte_plane(planes, G, t, (int)T.q[j], n0, full, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = j == 0 ? v[k] : m[k] + v[k];
        }
    }
    if (matte) {
        uint32_t a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = matte_q8(fminf(fmaxf(m[k], 0.f), 1.f));
        if (full) *(uint32_t*)(matte + n0) = a[0] | a[1] << 8 | a[2] << 16 | a[3] << 24;
        else
            for (int k = 0; k < 4 && n0 + k < N; ++k) matte[n0 + k] = (uint8_t)a[k];
    }
    if (mode == MATTE_ALPHA) return;

    uint32_t px[12];                                                  // the frame's bytes: pixel k, channel c at 3 k + c
    if (fflat && full) {
        const uint32_t* w = (const uint32_t*)(frame + 3 * n0);
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
        px[0] = w0 & 255; px[1] = (w0 >> 8) & 255; px[2] = (w0 >> 16) & 255; px[3] = w0 >> 24;
        px[4] = w1 & 255; px[5] = (w1 >> 8) & 255; px[6] = (w1 >> 16) & 255; px[7] = w1 >> 24;
        px[8] = w2 & 255; px[9] = (w2 >> 8) & 255; px[10] = (w2 >> 16) & 255; px[11] = w2 >> 24;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint8_t* s = frame + (long)t.oy[k] * ldf + 3l * t.ox[k];
            px[3 * k] = s[0]; px[3 * k + 1] = s[1]; px[3 * k + 2] = s[2];
        }
    }
    uint32_t side[4] = {0u, 0u, 0u, 0u};                              // hard modes: the pixel's id; layer: its R | G << 8 | B << 16 | A << 24
    if (mode <= MATTE_FADE) {
        if (full) {
            const uint32_t w = *(const uint32_t*)(ids + n0);
            side[0] = w & 255; side[1] = (w >> 8) & 255; side[2] = (w >> 16) & 255; side[3] = w >> 24;
        } else
            for (int k = 0; k < 4 && n0 + k < N; ++k) side[k] = ids[n0 + k];
    } else if (mode == MATTE_LAYER) {
        if (full) {
            const uint4 w = *(const uint4*)(layer + 4 * n0);
            side[0] = w.x; side[1] = w.y; side[2] = w.z; side[3] = w.w;
        } else
            for (int k = 0; k < 4 && n0 + k < N; ++k) side[k] = *(const uint32_t*)(layer + 4 * (n0 + k));
    }

    uint32_t o[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float im0 = matte_u8f(px[3 * k]), im1 = matte_u8f(px[3 * k + 1]), im2 = matte_u8f(px[3 * k + 2]);
        float x0, x1, x2;
        if (mode <= MATTE_FADE) {
            const uint32_t id = side[k];
            if (id) {
                const uint32_t c = ctab[id];
                x0 = im0 * ca + cb * matte_u8f(c & 255u);
                x1 = im1 * ca + cb * matte_u8f((c >> 8) & 255u);
                x2 = im2 * ca + cb * matte_u8f((c >> 16) & 255u);
            } else if (mode == MATTE_FADE) {
                x0 = im0 * 0.6f; x1 = im1 * 0.6f; x2 = im2 * 0.6f;
            } else { x0 = im0; x1 = im1; x2 = im2; }
        } else if (mode == MATTE_POPUP) {
            const float g = (im0 * 0.3f + im1 * 0.59f) + im2 * 0.11f, mm = m[k], rm = 1.0f - mm;
            x0 = mm * im0 + rm * g;
            x1 = mm * im1 + rm * g;
            x2 = mm * im2 + rm * g;
        } else {
            const uint32_t L = side[k];
            const float la = matte_u8f(L >> 24), mm = m[k], rm = 1.0f - mm, ba = rm * (1.0f - la);
            x0 = (im0 * ba + (matte_u8f(L & 255u) * rm) * la) + im0 * mm;
            x1 = (im1 * ba + (matte_u8f((L >> 8) & 255u) * rm) * la) + im1 * mm;
            x2 = (im2 * ba + (matte_u8f((L >> 16) & 255u) * rm) * la) + im2 * mm;
            x0 = fminf(fmaxf(x0, 0.f), 1.f); x1 = fminf(fmaxf(x1, 0.f), 1.f); x2 = fminf(fmaxf(x2, 0.f), 1.f);
        }
        o[3 * k] = matte_q8(x0); o[3 * k + 1] = matte_q8(x1); o[3 * k + 2] = matte_q8(x2);
    }
    if (full) {
        uint32_t* w = (uint32_t*)(out + 3 * n0);
        w[0] = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
        w[1] = o[4] | o[5] << 8 | o[6] << 16 | o[7] << 24;
        w[2] = o[8] | o[9] << 8 | o[10] << 16 | o[11] << 24;
    } else {
        for (int k = 0; k < 4 && n0 + k < N; ++k) {
            uint8_t* d = out + 3 * (n0 + k);
            d[0] = (uint8_t)o[3 * k]; d[1] = (uint8_t)o[3 * k + 1]; d[2] = (uint8_t)o[3 * k + 2];
        }
    }
}

// the planes 1 .. P - 1 quantised: out [P - 1, OH, OW].  A plane's first byte is dword-aligned iff (q - 1) * OH * OW is a multiple of 4.
extern "C" __global__ __launch_bounds__(256) void matte_soft_kernel(const float* __restrict__ planes, MatteGeom G, uint8_t* __restrict__ out) {
    const long N = (long)G.OH * G.OW, n0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (n0 >= N) return;
    const bool full = n0 + 4 <= N;
    MattePix t;
    matte_pixels(G, n0, N, t);
    for (int q = 1; q < G.P; ++q) {
        float v[4];
        matte_plane(planes, G, t, q, n0, full, v);
        const uint32_t a0 = matte_q8(v[0]), a1 = matte_q8(v[1]), a2 = matte_q8(v[2]), a3 = matte_q8(v[3]);
        uint8_t* d = out + (long)(q - 1) * N + n0;
        if (full && (((long)(q - 1) * N) & 3) == 0) *(uint32_t*)d = a0 | a1 << 8 | a2 << 16 | a3 << 24;
        else {
            const uint32_t a[4] = {a0, a1, a2, a3};
            for (int k = 0; k < 4 && n0 + k < N; ++k) d[k] = (uint8_t)a[k];
        }
    }
}

// what both stages check of the planes; -> 0 or the error code
static int matte_geometry(const char* who, const cutie_op* op, bool planes, MatteGeom& G) {
    const int32_t* i = op->i;
    const uint64_t* p = op->p;
    G.P = i[0]; G.H = i[1]; G.W = i[2]; G.plane = (long)i[3]; G.ldrow = i[4]; G.OH = i[5]; G.OW = i[6];
    if (G.OH < 1 || G.OW < 1) { cutie_set_error("%s: empty output (OH, OW >= 1)", who); return -2; }
    if (3l * G.OH * G.OW >= (1l << 31)) { cutie_set_error("%s: an output of %d x %d exceeds 2^31 bytes", who, G.OH, G.OW); return -2; }
    G.resample = 0; G.pflat = 0;
    if (!planes) return 0;
    if (G.H < 1 || G.W < 1) { cutie_set_error("%s: empty planes (H, W >= 1)", who); return -2; }
    if ((long)G.H * G.W >= (1l << 31)) { cutie_set_error("%s: planes of %d x %d exceed 2^31 pixels", who, G.H, G.W); return -2; }
    if (G.P < 1 || G.P > 256) { cutie_set_error("%s: %d planes, 1 <= P <= 256", who, G.P); return -2; }
    if ((long)G.P * G.OH * G.OW >= (1l << 31)) { cutie_set_error("%s: %d planes of %d x %d exceed 2^31 samples", who, G.P, G.OH, G.OW); return -2; }
    if (!p[0]) { cutie_set_error("%s: needs the planes (p0)", who); return -2; }
    if (p[0] & 3) { cutie_set_error("%s: planes (p0) 4-byte aligned", who); return -2; }
    if (G.ldrow < G.W || G.plane < 0) { cutie_set_error("%s: a row stride of %d elements, needs W = %d (and a plane stride >= 0)", who, G.ldrow, G.W); return -2; }
    G.resample = G.H != G.OH || G.W != G.OW;
    G.pflat = !G.resample && G.ldrow == G.W && (G.plane & 3) == 0 && (p[0] & 15) == 0;
    return 0;
}

// PROB_TO_ID flags == 256 (slots: include/cutie_hip.h, ABI 11, forms added)
int launch_matte_composite(const cutie_op* op, hipStream_t s) {
    const char* who = "matte composite";
    const int32_t* i = op->i;
    const uint64_t* p = op->p;
    const int mode = i[8], n = i[9], ldf = i[7];
    if (mode < MATTE_DAVIS || mode > MATTE_ALPHA) { cutie_set_error("%s: unknown mode %d (0 davis, 1 light, 2 fade, 3 popup, 4 layer, 5 alpha)", who, mode); return -2; }
    const bool soft = mode >= MATTE_POPUP;
    MatteGeom G;
    const int rc = matte_geometry(who, op, soft, G);
    if (rc) return rc;
    MatteTargets T;
    T.n = 0;
    if (soft) {
        if (n < 0 || n > MATTE_MAX_TARGETS) { cutie_set_error("%s: %d targets, 0 .. %d", who, n, MATTE_MAX_TARGETS); return -2; }
        if (n > 0 && !p[1]) { cutie_set_error("%s: needs the target list (p1, host memory)", who); return -2; }
        if (p[1] & 3) { cutie_set_error("%s: target list (p1) 4-byte aligned", who); return -2; }
        const int32_t* tg = (const int32_t*)p[1];
        for (int j = 0; j < n; ++j) {
            if (tg[j] < 0 || tg[j] >= G.P) { cutie_set_error("%s: target %d is plane %d, 0 .. P - 1 = %d", who, j, tg[j], G.P - 1); return -2; }
            T.q[j] = (uint8_t)tg[j];
        }
        T.n = n;
    } else if (p[4]) { cutie_set_error("%s: the matte plane (p4) needs a soft mode (popup, layer, alpha)", who); return -2; }
    if (mode == MATTE_ALPHA && !p[4]) { cutie_set_error("%s: mode alpha needs the matte plane (p4)", who); return -2; }
    if (p[4] & 15) { cutie_set_error("%s: matte plane (p4) 16-byte aligned", who); return -2; }
    if (mode != MATTE_ALPHA) {
        if (!p[2] || !p[3]) { cutie_set_error("%s: needs the frame (p2) and the output frame (p3)", who); return -2; }
        if (p[3] & 15) { cutie_set_error("%s: output frame (p3) 16-byte aligned", who); return -2; }
        if ((long)ldf < 3l * G.OW) { cutie_set_error("%s: frame row stride of %d bytes, needs 3 OW = %ld", who, ldf, 3l * G.OW); return -2; }
        if (!soft) {
            if (!p[5] || !p[6]) { cutie_set_error("%s: modes davis, light and fade need the id plane (p5) and the colour table (p6)", who); return -2; }
            if ((p[5] & 3) || (p[6] & 3)) { cutie_set_error("%s: id plane (p5) and colour table (p6) 4-byte aligned", who); return -2; }
        }
        if (mode == MATTE_LAYER) {
            if (!p[7]) { cutie_set_error("%s: mode layer needs the layer (p7)", who); return -2; }
            if (p[7] & 15) { cutie_set_error("%s: layer (p7) 16-byte aligned", who); return -2; }
        }
    }
    const double alpha = mode == MATTE_LIGHT ? 0.9 : 0.5;
    const int fflat = (long)ldf == 3l * G.OW && (p[2] & 3) == 0;
    const long groups = ((long)G.OH * G.OW + 3) / 4;
    hipLaunchKernelGGL(matte_composite_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, s, (const float*)p[0], G, T, (const uint8_t*)p[2],
                       (long)ldf, fflat, (const uint8_t*)p[5], (const uint32_t*)p[6], (const uint8_t*)p[7], (uint8_t*)p[3], (uint8_t*)p[4], mode,
                       (float)alpha, (float)(1.0 - alpha));
    return (int)hipGetLastError();
}

// PROB_TO_ID flags == 512 (slots: include/cutie_hip.h, ABI 11, forms added)
int launch_matte_soft(const cutie_op* op, hipStream_t s) {
    const char* who = "matte soft";
    const uint64_t* p = op->p;
    MatteGeom G;
    const int rc = matte_geometry(who, op, true, G);
    if (rc) return rc;
    if (G.P == 1) return 0;                                           // no object plane: nothing to write
    if (!p[2]) { cutie_set_error("%s: needs the output planes (p2)", who); return -2; }
    if (p[2] & 15) { cutie_set_error("%s: output planes (p2) 16-byte aligned", who); return -2; }
    const long groups = ((long)G.OH * G.OW + 3) / 4;
    hipLaunchKernelGGL(matte_soft_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, s, (const float*)p[0], G, (uint8_t*)p[2]);
    return (int)hipGetLastError();
}
