// PROB_TO_ID flags == 1024 (ABI 11, form added): the per-object track statistics of a uint8 id plane [H, W] -- area, bounding box and
// the coordinate sums behind the centroid -- and, from the probability planes the ids were decided on, how sure the model was of every
// listed object: 12 integers per object leave the device instead of a mask (the float arithmetic on them and the files:
// cutie_amd/inference/utils/track_report.py; the numpy model of the table: tests/track_ref.py; slots: include/cutie_hip.h).
//
// Row k of the table belongs to objs[k]:  0 area | 1 xmin 2 ymin 3 xmax 4 ymax | 5,6 sum of x | 7,8 sum of y | 9 samples won | 10,11 sum of
// q16(winning probability); 64-bit values as (low, high) word pairs.  x = column, y = row of the id plane.
//
// Four launches:
//   1  trk_init_kernel   every row = (0, W, H, -1, -1, 0 ...): the identities of +, min and max (the launch WRITES the table)
//   2  trk_geom_kernel   one sweep over the id plane, 16 pixels (one 16-byte load where the plane allows it) per thread and round.  A thread
//                        keeps the sums of ONE object in registers -- background costs nothing, and 16 equal bytes inside a row are one
//                        step -- and spills them to the block's LDS rows when another listed object turns up.  What is left at the end is
//                        combined across the wave with shuffles, once per object the wave holds, and goes to LDS from one lane.  The block
//                        then issues one set of global integer atomics per object it met.
//   3  trk_conf_kernel   (p0 != 0) the same form over the samples of the probability planes: q* = the first largest plane (prob_to_id_kernel's
//                        loop: v > best from plane 0 on), row = that of lut[q*]; count += 1, sum += q16(prob[q*]).
//   4  trk_dup_kernel    an entry equal to an earlier one gets the earlier one's row (only launched for n > 1).
// Every sum is an integer sum and every min / max an integer min / max, gathered with integer atomics: the table depends on the planes, the
// lists and the lut alone, not on launch shape or timing.  Width of the accumulators: a thread, a block's LDS row and the table all hold the
// coordinate and probability sums in 64 bits (sum of x reaches H W (W - 1) / 2: beyond 2^32 from 513 x 4096 on); areas and counts are at
// most H W < 2^31.  The table's 64-bit values start at words 5 and 7, which are only 4-byte aligned, so they are added as two 32-bit
// atomics: the low word with its old value returned, and the high word by the carry that old value shows -- every wrap of the low word is
// seen by exactly one add, so the pair ends as the exact sum whatever the order.
#include "common.h"

#define TRK_WORDS 12
#define TRK_MAX_BLOCKS 1024              // grid-stride sweeps: at most this many blocks touch the table

__global__ __launch_bounds__(256) void trk_init_kernel(int* __restrict__ table, int n, int H, int W) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * TRK_WORDS) return;
    const int w = idx % TRK_WORDS;
    table[idx] = w == 1 ? W : w == 2 ? H : (w == 3 || w == 4) ? -1 : 0;
}

// id -> first row that lists it, -1 for an id nobody lists (entries outside 1 .. 255 list nothing)
__device__ __forceinline__ void trk_rows_of_ids(int* rows_s, const int* __restrict__ objs, int n, int t) {
    rows_s[t] = 0x7fffffff;
    __syncthreads();
    if (t < n) {
        const int v = objs[t];
        if (v >= 1 && v <= 255) atomicMin(&rows_s[v], t);      // the smallest t stays: an integer min, whatever the order
    }
    __syncthreads();
    if (rows_s[t] == 0x7fffffff) rows_s[t] = -1;               // (every thread rewrites its own entry only)
    __syncthreads();
}

// table[word], table[word + 1] += v as a 64-bit pair (see the head of the file)
__device__ __forceinline__ void trk_add_pair(int* __restrict__ word, unsigned long long v) {
    const unsigned lo = (unsigned)v;
    unsigned hi = (unsigned)(v >> 32);
    if (lo) {
        const unsigned old = atomicAdd((unsigned*)word, lo);
        if (old + lo < old) ++hi;
    }
    if (hi) atomicAdd((unsigned*)word + 1, hi);
}

struct TrkGeom {
    int k, area, xmin, ymin, xmax, ymax;
    unsigned long long sx, sy;
};

__device__ __forceinline__ void trk_geom_reset(TrkGeom& a, int k) {
    a.k = k;
    a.area = 0;
    a.xmin = a.ymin = 0x7fffffff;
    a.xmax = a.ymax = -1;
    a.sx = a.sy = 0ull;
}

// LDS rows: l32[k][5] = area, xmin, ymin, xmax, ymax; l64[k][2] = sum x, sum y
__device__ __forceinline__ void trk_geom_spill(int* l32, unsigned long long* l64, int k, int area, int xmin, int ymin, int xmax, int ymax,
                                               unsigned long long sx, unsigned long long sy) {
    atomicAdd(&l32[k * 5 + 0], area);
    atomicMin(&l32[k * 5 + 1], xmin);
    atomicMin(&l32[k * 5 + 2], ymin);
    atomicMax(&l32[k * 5 + 3], xmax);
    atomicMax(&l32[k * 5 + 4], ymax);
    atomicAdd(&l64[k * 2 + 0], sx);
    atomicAdd(&l64[k * 2 + 1], sy);
}

__device__ __forceinline__ unsigned long long trk_shfl_xor64(unsigned long long v, int off) {
    const unsigned lo = __shfl_xor((unsigned)v, off, 64), hi = __shfl_xor((unsigned)(v >> 32), off, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// launch 2.  chunks = ceil(H W / 16); vec: the plane starts on a 16-byte boundary (whole chunks are one load)
__global__ __launch_bounds__(256) void trk_geom_kernel(const uint8_t* __restrict__ ids, int H, int W, const int* __restrict__ objs, int n,
                                                       int vec, int* __restrict__ table) {
    __shared__ int rows_s[256];
    __shared__ int l32[255 * 5];
    __shared__ unsigned long long l64[255 * 2];
    const int t = threadIdx.x, lane = t & 63;
    trk_rows_of_ids(rows_s, objs, n, t);
    for (int idx = t; idx < n * 5; idx += 256) {
        const int w = idx % 5;
        l32[idx] = w == 0 ? 0 : (w <= 2 ? 0x7fffffff : -1);
    }
    for (int idx = t; idx < n * 2; idx += 256) l64[idx] = 0ull;
    __syncthreads();

    const long HW = (long)H * W;                               // < 2^31
    const long chunks = (HW + 15) >> 4;
    TrkGeom a;
    trk_geom_reset(a, -1);
    for (long c = (long)blockIdx.x * 256 + t; c < chunks; c += (long)gridDim.x * 256) {
        const long at = c << 4;
        const int left = (int)min(16l, HW - at);
        unsigned px[4] = {0u, 0u, 0u, 0u};                     // (bytes past the plane's end read as 0: nobody lists 0)
        if (vec && left == 16) {
            const uint4 v = *(const uint4*)(ids + at);
            px[0] = v.x; px[1] = v.y; px[2] = v.z; px[3] = v.w;
        } else {
            for (int j = 0; j < left; ++j) px[j >> 2] |= (unsigned)ids[at + j] << (8 * (j & 3));
        }
        if ((px[0] | px[1] | px[2] | px[3]) == 0u) continue;   // background only
        int y = (int)(at / W), x = (int)(at - (long)y * W);
        const unsigned b0 = px[0] & 255u;
        if (px[0] == b0 * 0x01010101u && px[1] == px[0] && px[2] == px[0] && px[3] == px[0] && x + 15 < W) {       // 16 pixels of one id in one row
            const int k = rows_s[b0];
            if (k < 0) continue;
            if (k != a.k) {
                if (a.area) trk_geom_spill(l32, l64, a.k, a.area, a.xmin, a.ymin, a.xmax, a.ymax, a.sx, a.sy);
                trk_geom_reset(a, k);
            }
            a.area += 16;
            a.sx += 16ull * (unsigned)x + 120ull;
            a.sy += 16ull * (unsigned)y;
            a.xmin = min(a.xmin, x);
            a.xmax = max(a.xmax, x + 15);
            a.ymin = min(a.ymin, y);
            a.ymax = max(a.ymax, y);
            continue;
        }
        for (int j = 0; j < left; ++j) {
            const int k = rows_s[(px[j >> 2] >> (8 * (j & 3))) & 255u];
            if (k >= 0) {
                if (k != a.k) {
                    if (a.area) trk_geom_spill(l32, l64, a.k, a.area, a.xmin, a.ymin, a.xmax, a.ymax, a.sx, a.sy);
                    trk_geom_reset(a, k);
                }
                a.area += 1;
                a.sx += (unsigned)x;
                a.sy += (unsigned)y;
                a.xmin = min(a.xmin, x);
                a.xmax = max(a.xmax, x);
                a.ymin = min(a.ymin, y);
                a.ymax = max(a.ymax, y);
            }
            if (++x == W) { x = 0; ++y; }
        }
    }
    // what the lanes still hold: one round per object of the wave (the loop's condition is the same in every lane)
    unsigned long long pend = __ballot(a.area > 0);
    while (pend) {
        const int kk = __shfl(a.k, __ffsll((long long)pend) - 1, 64);
        const bool mine = a.area > 0 && a.k == kk;
        int area = mine ? a.area : 0, xmin = mine ? a.xmin : 0x7fffffff, ymin = mine ? a.ymin : 0x7fffffff, xmax = mine ? a.xmax : -1, ymax = mine ? a.ymax : -1;
        unsigned long long sx = mine ? a.sx : 0ull, sy = mine ? a.sy : 0ull;
        for (int off = 32; off > 0; off >>= 1) {
            area += __shfl_xor(area, off, 64);
            xmin = min(xmin, __shfl_xor(xmin, off, 64));
            ymin = min(ymin, __shfl_xor(ymin, off, 64));
            xmax = max(xmax, __shfl_xor(xmax, off, 64));
            ymax = max(ymax, __shfl_xor(ymax, off, 64));
            sx += trk_shfl_xor64(sx, off);
            sy += trk_shfl_xor64(sy, off);
        }
        if (lane == 0) trk_geom_spill(l32, l64, kk, area, xmin, ymin, xmax, ymax, sx, sy);
        pend &= ~__ballot(mine);
    }
    __syncthreads();
    if (t < n && l32[t * 5] > 0) {                             // one set of global atomics per object the block met
        int* row = table + t * TRK_WORDS;
        atomicAdd(row + 0, l32[t * 5 + 0]);
        atomicMin(row + 1, l32[t * 5 + 1]);
        atomicMin(row + 2, l32[t * 5 + 2]);
        atomicMax(row + 3, l32[t * 5 + 3]);
        atomicMax(row + 4, l32[t * 5 + 4]);
        trk_add_pair(row + 5, l64[t * 2 + 0]);
        trk_add_pair(row + 7, l64[t * 2 + 1]);
    }
}

// q16 of include/cutie_hip.h: NaN and everything not above 0 count as 0
__device__ __forceinline__ unsigned trk_q16(float v) {
    if (!(v > 0.f)) return 0u;
    if (v >= 1.f) return 65535u;
    return (unsigned)(int)(v * 65535.f + 0.5f);
}

// launch 3: one sample per thread and round
__global__ __launch_bounds__(256) void trk_conf_kernel(const float* __restrict__ prob, const int* __restrict__ lut, int P, int h, int w, long plane,
                                                       int ldrow, const int* __restrict__ objs, int n, int* __restrict__ table) {
    __shared__ int rows_s[256];
    __shared__ int prow_s[256];                                // plane -> row of the object it stands for, -1: not listed
    __shared__ int lcnt[255];
    __shared__ unsigned long long lsum[255];
    const int t = threadIdx.x, lane = t & 63;
    trk_rows_of_ids(rows_s, objs, n, t);
    {
        const int id = t < P ? lut[t] : -1;
        prow_s[t] = (id >= 0 && id <= 255) ? rows_s[id] : -1;
    }
    if (t < n) { lcnt[t] = 0; lsum[t] = 0ull; }
    __syncthreads();

    const long hw = (long)h * w;                               // < 2^31
    int ak = -1, acnt = 0;
    unsigned long long asum = 0ull;
    for (long idx = (long)blockIdx.x * 256 + t; idx < hw; idx += (long)gridDim.x * 256) {
        const int yy = (int)(idx / w), xx = (int)(idx - (long)yy * w);
        const float* src = prob + (long)yy * ldrow + xx;
        float best = src[0];
        int arg = 0;
        for (int q = 1; q < P; ++q) {
            const float v = src[(long)q * plane];
            if (v > best) { best = v; arg = q; }
        }
        const int k = prow_s[arg];
        if (k < 0) continue;
        if (k != ak) {
            if (acnt) { atomicAdd(&lcnt[ak], acnt); atomicAdd(&lsum[ak], asum); }
            ak = k; acnt = 0; asum = 0ull;
        }
        acnt += 1;
        asum += trk_q16(best);
    }
    unsigned long long pend = __ballot(acnt > 0);
    while (pend) {
        const int kk = __shfl(ak, __ffsll((long long)pend) - 1, 64);
        const bool mine = acnt > 0 && ak == kk;
        int cnt = mine ? acnt : 0;
        unsigned long long sum = mine ? asum : 0ull;
        for (int off = 32; off > 0; off >>= 1) {
            cnt += __shfl_xor(cnt, off, 64);
            sum += trk_shfl_xor64(sum, off);
        }
        if (lane == 0) { atomicAdd(&lcnt[kk], cnt); atomicAdd(&lsum[kk], sum); }
        pend &= ~__ballot(mine);
    }
    __syncthreads();
    if (t < n && lcnt[t] > 0) {
        int* row = table + t * TRK_WORDS;
        atomicAdd(row + 9, lcnt[t]);
        trk_add_pair(row + 10, lsum[t]);
    }
}

// launch 4: thread (k, word); an entry that repeats an earlier one reads the earlier one's row (which no thread of this launch writes)
__global__ __launch_bounds__(256) void trk_dup_kernel(const int* __restrict__ objs, int n, int* __restrict__ table) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * TRK_WORDS) return;
    const int k = idx / TRK_WORDS, w = idx - k * TRK_WORDS;
    const int v = objs[k];
    if (v < 1 || v > 255) return;
    for (int e = 0; e < k; ++e)
        if (objs[e] == v) { table[idx] = table[e * TRK_WORDS + w]; return; }
}

// PROB_TO_ID flags == 1024.  p2 = ids u8 [i1, i2], p6 = object ids int32 [i9], p7 = table int32 [i9, 12]; optional p0 = planes f32
// (i0 planes of i5 x i6, plane stride i3, row stride i4), p1 = lut int32 [i0]
int launch_track_stats(const cutie_op* op, hipStream_t s) {
    const uint64_t* p = op->p;
    const int H = op->i[1], W = op->i[2], n = op->i[9];
    if (H < 1 || W < 1) { cutie_set_error("track stats: empty shape (H, W >= 1)"); return -2; }
    if ((long)H * W >= (1l << 31)) { cutie_set_error("track stats: %d x %d exceeds 2^31 pixels", H, W); return -2; }
    if (n < 0 || n > 255) { cutie_set_error("track stats: %d objects, 0 <= n <= 255", n); return -2; }
    if (!p[2]) { cutie_set_error("track stats: needs the id plane (p2)"); return -2; }
    const bool conf = p[0] != 0;
    if (conf) {
        const int P = op->i[0], h = op->i[5], w = op->i[6];
        if (P < 1 || P > 256) { cutie_set_error("track stats: %d probability planes, 1 <= P <= 256", P); return -2; }
        if (h < 1 || w < 1) { cutie_set_error("track stats: empty probability planes (h, w >= 1)"); return -2; }
        if ((long)h * w >= (1l << 31)) { cutie_set_error("track stats: planes of %d x %d exceed 2^31 samples", h, w); return -2; }
        if (op->i[4] < w || op->i[3] < 0) { cutie_set_error("track stats: row stride %d below the row of %d samples, or a negative plane stride", op->i[4], w); return -2; }
        if (!p[1]) { cutie_set_error("track stats: probability planes (p0) need the lut (p1)"); return -2; }
        if ((p[0] & 3) || (p[1] & 3)) { cutie_set_error("track stats: probability planes and lut 4-byte aligned"); return -2; }
    }
    if (n == 0) return 0;                                      // nothing to write
    if (!p[6] || !p[7]) { cutie_set_error("track stats: needs the object ids (p6) and the table (p7)"); return -2; }
    if ((p[6] & 3) || (p[7] & 15)) { cutie_set_error("track stats: object ids 4-byte aligned, table 16-byte aligned"); return -2; }
    const int* objs = (const int*)p[6];
    int* table = (int*)p[7];
    const int words = n * TRK_WORDS;
    hipLaunchKernelGGL(trk_init_kernel, dim3((words + 255) / 256), dim3(256), 0, s, table, n, H, W);
    const long chunks = ((long)H * W + 15) >> 4;
    const unsigned gblocks = (unsigned)min((chunks + 255) / 256, (long)TRK_MAX_BLOCKS);
    hipLaunchKernelGGL(trk_geom_kernel, dim3(gblocks), dim3(256), 0, s, (const uint8_t*)p[2], H, W, objs, n, (int)((p[2] & 15) == 0), table);
    if (conf) {
        const long hw = (long)op->i[5] * op->i[6];
        const unsigned cblocks = (unsigned)min((hw + 255) / 256, (long)TRK_MAX_BLOCKS);
        hipLaunchKernelGGL(trk_conf_kernel, dim3(cblocks), dim3(256), 0, s, (const float*)p[0], (const int*)p[1], op->i[0], op->i[5], op->i[6], (long)op->i[3],
                           op->i[4], objs, n, table);
    }
    if (n > 1) hipLaunchKernelGGL(trk_dup_kernel, dim3((words + 255) / 256), dim3(256), 0, s, objs, n, table);
    return (int)hipGetLastError();
}
