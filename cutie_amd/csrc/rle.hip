// PROB_TO_ID flags == 32 (ABI 9): COCO compressed-RLE strings of the objects of a uint8 id plane [H, W], made on the device -- what the
// BURST json carries per object (ResultSaver egress='device' with init_json, cutie_amd/inference/utils/results_utils.py; the format and the
// numpy model whose bytes these are: cutie_amd/inference/utils/coco_rle.py).
//
// The mask of object k is (id == objs[k]), flattened COLUMN-major: position p = x * H + y.  Its counts are the distances between its run
// boundaries, a run of zeros first; count j > 2 is coded as counts[j] - counts[j - 2]; every value as 5-bit groups + 48.
//
// One sweep serves all objects.  With id[-1] = 0, a transition id[p] != id[p-1] starts a run of ones of the listed object id[p] and ends
// the run of the listed object id[p-1]; the starts and ends of ONE object alternate, so the r-th start of object k is its boundary 2r and
// the end of that run its boundary 2r + 1: only the starts are ranked.  The plane is row-major, the order column-major: a block reads a
// tile of RLE_TC columns x RLE_SEG rows along the rows and turns it in LDS; a CHUNK is one column of a tile (<= RLE_SEG consecutive
// positions), chunk number = x * nseg + segment, ascending with p.
//
// Six launches, 256 threads each; a grid-wide dependency (a scan) lies between any two:
//   1  rle_sweep_kernel<false>  per chunk and object: the number of starts -> cnt[k][chunk]
//   2  rle_chunkscan_kernel     one block per object: exclusive scan of its row of cnt, total S_k; clears the object's accumulators
//   3  rle_sweep_kernel<true>   the same walk; a wave takes 64 positions per step and ranks the starts of equal objects among its lanes
//                               with 8 ballots (the slot number bit by bit); boundary positions go to B: object k owns 2 S_k + 1 words at
//                               base_k = sum over k' < k of (2 S_k' + 1), the last one the sentinel H * W
//   4  rle_len_kernel           one thread per 4 boundaries: count = B[j] - B[j-1] (B[-1] = 0; the sentinel's count is dropped when it is
//                               0: the last run ended at H * W), difference, number of characters; sums per 1024 boundaries, and per
//                               object bytes / area by integer atomics -- in LDS first, then one global atomic per object and block
//                               (sums of integers: the same in any order; per-thread global atomics on a few addresses cost 0.75 ms at 720p)
//   5  rle_finish_kernel        one block: scan of the objects' bytes -> the table, capacity check -> the status, scan of the block sums
//   6  rle_emit_kernel          recomputes 4, scans inside the block and writes the characters (byte stores) at their offsets
// Every offset comes from a scan over a fixed order (object, then position): the bytes depend on the plane and the object list alone.
#include "common.h"

#define RLE_SEG 256                      // rows of a tile = the longest chunk
#define RLE_TC 16                        // columns of a tile
#define RLE_PITCH (RLE_SEG + 4)          // bytes between two columns of the tile in LDS
#define RLE_NONE 255                     // slot of an id that is not listed (slots are 0 .. 254)
#define RLE_PER_BLOCK 1024               // boundaries per block of launches 4 and 6 (4 per thread)
#define RLE_HDR 1024                     // scratch, first words: S_k [256] | bytes per object u64 [256] | area per object [256]
#define RLE_BYTES 256
#define RLE_AREA 768

static long rle_nblk(long HW, int n) { return (2 * HW + n + RLE_PER_BLOCK - 1) / RLE_PER_BLOCK; }

// exclusive scan of v over the 256 threads of the block (all of them call it), the sum to every thread; red = 4 words of LDS
__device__ __forceinline__ int rle_scan256(int v, int* red, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    __syncthreads();                                          // (the previous use of red is over)
    if (lane == 63) red[w] = inc;
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = red[q];
        if (q < w) pre += r;
        tot += r;
    }
    total = tot;
    return pre + inc - v;
}

// lanes whose key equals `key`, from the ballots of the keys' 8 bits (a lane without a start has the key RLE_NONE = all bits set)
__device__ __forceinline__ uint64_t rle_match(const uint64_t* bal, int key) {
    uint64_t m = ~0ull;
#pragma unroll
    for (int b = 0; b < 8; ++b) m &= ((key >> b) & 1) ? bal[b] : ~bal[b];
    return m;
}

// launches 1 and 3: grid = column tiles x row segments
template <bool FILL>
__global__ __launch_bounds__(256) void rle_sweep_kernel(const uint8_t* __restrict__ ids, int H, int W, const int* __restrict__ objs, int n, int nseg,
                                                        int* __restrict__ cnt, int* __restrict__ hdr, int* __restrict__ B, int G) {
    __shared__ uint8_t tile[RLE_TC * RLE_PITCH];
    __shared__ uint8_t slot[256];
    __shared__ uint8_t pred[RLE_TC];
    __shared__ int objs_s[256];
    __shared__ int ctr_s[4][256];
    __shared__ int base[256];
    __shared__ int red[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int tx = blockIdx.x / nseg, s = blockIdx.x % nseg;
    const int x0 = tx * RLE_TC, y0 = s * RLE_SEG;
    const long nchunk = (long)W * nseg;
    const int N = H * W;
    objs_s[t] = t < n ? objs[t] : -1;
    for (int idx = t; idx < RLE_TC * RLE_SEG; idx += 256) {   // along the rows: 16 neighbouring threads read 16 neighbouring bytes
        const int r = idx / RLE_TC, c = idx % RLE_TC;
        const int y = y0 + r, x = x0 + c;
        tile[c * RLE_PITCH + r] = (y < H && x < W) ? ids[(long)y * W + x] : (uint8_t)0;
    }
    if (t < RLE_TC) {                                         // what precedes a chunk: the row above, the bottom of the column before, or id[-1] = 0
        const int x = x0 + t;
        uint8_t v = 0;
        if (x < W) {
            if (y0 > 0) v = ids[(long)(y0 - 1) * W + x];
            else if (x > 0) v = ids[(long)(H - 1) * W + x - 1];
        }
        pred[t] = v;
    }
    int S_t = 0;
    if (FILL) {
        S_t = t < n ? hdr[t] : 0;
        int total;
        base[t] = rle_scan256(t < n ? 2 * S_t + 1 : 0, red, total);
    }
    __syncthreads();
    {                                                          // id -> slot: the first place of the list that names it; 0 is never an object
        int sl = RLE_NONE;
        if (t > 0)
            for (int k = n - 1; k >= 0; --k)
                if (objs_s[k] == t) sl = k;
        slot[t] = (uint8_t)sl;
    }
    __syncthreads();
    if (FILL && blockIdx.x == 0) {                             // the sentinels, the end of a run that reaches the last pixel, the total
        if (t < n) {
            const int at = base[t] + 2 * S_t;
            if ((unsigned)at < (unsigned)G) B[at] = N;
        }
        if (t == 0) {
            const int sl = slot[ids[(long)N - 1]];
            if (sl != RLE_NONE) {
                const int at = base[sl] + 2 * hdr[sl] - 1;
                if (at >= 0 && at < G) B[at] = N;
            }
        }
    }
    volatile int* ctr = ctr_s[w];                              // the wave's running number of starts per object
    const uint64_t below = (1ull << lane) - 1ull;
    for (int c = w; c < RLE_TC; c += 4) {                      // a wave takes every fourth column of the tile
        const int x = x0 + c;
        if (x >= W) break;
        const int rows = min(RLE_SEG, H - y0);
        const long chunk = (long)x * nseg + s;
        for (int k = lane; k < n; k += 64) ctr[k] = FILL ? cnt[k * nchunk + chunk] : 0;
        const uint8_t* col = tile + c * RLE_PITCH;
        for (int r0 = 0; r0 < rows; r0 += 64) {
            const int r = r0 + lane;
            const bool in = r < rows;
            const int b = in ? col[r] : 0, a = in ? (r > 0 ? col[r - 1] : pred[c]) : 0;
            const bool trans = in && a != b;
            const int kb = trans ? slot[b] : RLE_NONE, ka = trans ? slot[a] : RLE_NONE;
            uint64_t bal[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) bal[q] = __ballot((kb >> q) & 1);
            const int p = x * H + y0 + r;
            uint64_t peers = 0;
            int first = 0;
            if (kb != RLE_NONE) {                              // a start: boundary 2 r of its object
                peers = rle_match(bal, kb);
                first = __popcll(peers & below);
                if (FILL) {
                    const int at = base[kb] + 2 * (ctr[kb] + first);
                    if ((unsigned)at < (unsigned)G) B[at] = p;
                }
            }
            if (FILL && ka != RLE_NONE) {                      // an end: the boundary behind the latest start of its object
                const int starts = ctr[ka] + __popcll(rle_match(bal, ka) & below);
                const int at = base[ka] + 2 * starts - 1;
                if (starts > 0 && (unsigned)at < (unsigned)G) B[at] = p;
            }
            if (kb != RLE_NONE && first == 0) ctr[kb] += __popcll(peers);     // one lane per object, after every lane has read
        }
        if (!FILL)
            for (int k = lane; k < n; k += 64) cnt[k * nchunk + chunk] = ctr[k];
    }
}

// launch 2: grid = n objects
__global__ __launch_bounds__(256) void rle_chunkscan_kernel(int* __restrict__ cnt, long nchunk, int* __restrict__ hdr) {
    __shared__ int red[4];
    const int k = blockIdx.x, t = threadIdx.x;
    int* row = cnt + k * nchunk;
    int carry = 0;
    for (long c0 = 0; c0 < nchunk; c0 += 256) {
        const long c = c0 + t;
        const int v = c < nchunk ? row[c] : 0;
        int total;
        const int ex = rle_scan256(v, red, total);
        if (c < nchunk) row[c] = carry + ex;
        carry += total;
    }
    if (t == 0) {
        hdr[k] = carry;
        ((unsigned long long*)(hdr + RLE_BYTES))[k] = 0ull;
        hdr[RLE_AREA + k] = 0;
    }
}

// what launches 4 and 6 share: the object tables in LDS and the value of boundary g
struct RleObjs {
    int base[257];
    int S[256];
    int red[4];
};

__device__ __forceinline__ int rle_load_objs(RleObjs& o, const int* __restrict__ hdr, int n) {
    const int t = threadIdx.x;
    const int S = t < n ? hdr[t] : 0;
    int G;
    const int ex = rle_scan256(t < n ? 2 * S + 1 : 0, o.red, G);
    o.base[t] = ex;
    o.S[t] = S;
    if (t == 0) o.base[256] = G;
    __syncthreads();
    return G;
}

// boundary g (< G) -> its object k, its count (< 0: the dropped sentinel count) and the coded value
__device__ __forceinline__ void rle_value(const RleObjs& o, const int* __restrict__ B, int n, int g, int& k, int& j, int& count, int& value) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (o.base[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    k = lo;
    j = g - o.base[k];
    const int* Bk = B + o.base[k];
    const int c = Bk[j] - (j > 0 ? Bk[j - 1] : 0);
    count = (j > 0 && j == 2 * o.S[k] && c == 0) ? -1 : c;
    value = j > 2 ? c - (Bk[j - 2] - Bk[j - 3]) : c;
}

__device__ __forceinline__ int rle_nchars(int x) {
    int nch = 0;
    bool more = true;
    while (more) {
        const int c = x & 0x1f;
        x >>= 5;
        more = (c & 0x10) ? x != -1 : x != 0;
        ++nch;
    }
    return nch;                                                // <= 7 for 32 bits
}

// launch 4: grid = blocks of RLE_PER_BLOCK boundaries (sized for the largest G, 2 H W + n; the blocks behind G leave at once)
__global__ __launch_bounds__(256) void rle_len_kernel(const int* __restrict__ B, int* __restrict__ hdr, int n, int* __restrict__ blocksum) {
    __shared__ RleObjs o;
    __shared__ int lbytes[256], larea[256];                   // the block's share per object: LDS atomics first, one global atomic per object and block
    lbytes[threadIdx.x] = 0;
    larea[threadIdx.x] = 0;
    const int G = rle_load_objs(o, hdr, n);
    const long g0 = (long)blockIdx.x * RLE_PER_BLOCK + threadIdx.x * 4;
    if ((long)blockIdx.x * RLE_PER_BLOCK >= G) return;
    int sum = 0, curk = -1, bytes = 0, area = 0;
    for (int q = 0; q < 4; ++q) {
        const long g = g0 + q;
        if (g >= G) break;
        int k, j, count, value;
        rle_value(o, B, n, (int)g, k, j, count, value);
        if (k != curk) {
            if (curk >= 0) { atomicAdd(lbytes + curk, bytes); if (area) atomicAdd(larea + curk, area); }
            curk = k; bytes = 0; area = 0;
        }
        if (count < 0) continue;
        const int nch = rle_nchars(value);
        sum += nch;
        bytes += nch;
        if (j & 1) area += count;
    }
    if (curk >= 0) { atomicAdd(lbytes + curk, bytes); if (area) atomicAdd(larea + curk, area); }
    int total;
    rle_scan256(sum, o.red, total);                           // (its barriers also close the LDS atomics)
    if (threadIdx.x == 0) blocksum[blockIdx.x] = total;
    if (lbytes[threadIdx.x]) atomicAdd((unsigned long long*)(hdr + RLE_BYTES) + threadIdx.x, (unsigned long long)lbytes[threadIdx.x]);
    if (larea[threadIdx.x]) atomicAdd(hdr + RLE_AREA + threadIdx.x, larea[threadIdx.x]);
}

// launch 5: one block.  table[k] = {byte offset, bytes, counts, area}; status = {bytes of all strings, error bits, counts of all strings, 0}
__global__ __launch_bounds__(256) void rle_finish_kernel(const int* __restrict__ B, int* __restrict__ hdr, int n, int HW, int* __restrict__ blocksum,
                                                         int4* __restrict__ table, int* __restrict__ status, int cap) {
    __shared__ RleObjs o;
    __shared__ unsigned long long wide[4];
    const int t = threadIdx.x;
    const int G = rle_load_objs(o, hdr, n);
    const unsigned long long mine = t < n ? ((const unsigned long long*)(hdr + RLE_BYTES))[t] : 0ull;
    unsigned long long all = mine;                            // the total in 64 bits (a plane of noise can pass 2^31 bytes: it fits no capacity)
    for (int off = 32; off > 0; off >>= 1) all += __shfl_xor(all, off, 64);
    if ((t & 63) == 0) wide[t >> 6] = all;
    __syncthreads();
    all = wide[0] + wide[1] + wide[2] + wide[3];
    const bool fits = all <= (unsigned long long)cap;
    int total;
    const int off = rle_scan256(fits ? (int)mine : 0, o.red, total);
    int counts = 0;
    if (t < n) {
        const int S = o.S[t];
        counts = 2 * S + 1 - ((S > 0 && B[o.base[t] + 2 * S - 1] == HW) ? 1 : 0);
    }
    int ncounts;
    rle_scan256(counts, o.red, ncounts);
    if (t < n) table[t] = make_int4(fits ? off : 0, (int)(mine < 0x7fffffffull ? mine : 0x7fffffffull), counts, hdr[RLE_AREA + t]);
    if (t == 0) {
        status[0] = (int)(all < 0x7fffffffull ? all : 0x7fffffffull);
        status[1] = fits ? 0 : 1;
        status[2] = ncounts;
        status[3] = 0;
    }
    if (!fits) return;
    const int nact = (G + RLE_PER_BLOCK - 1) / RLE_PER_BLOCK;
    int carry = 0;
    for (int b0 = 0; b0 < nact; b0 += 256) {
        const int b = b0 + t;
        const int v = b < nact ? blocksum[b] : 0;
        int tot;
        const int ex = rle_scan256(v, o.red, tot);
        if (b < nact) blocksum[b] = carry + ex;
        carry += tot;
    }
}

// launch 6: grid as launch 4
__global__ __launch_bounds__(256) void rle_emit_kernel(const int* __restrict__ B, const int* __restrict__ hdr, int n, const int* __restrict__ blocksum,
                                                       const int* __restrict__ status, uint8_t* __restrict__ out, int cap) {
    __shared__ RleObjs o;
    if (status[1] != 0) return;                               // it does not fit: nothing is written
    const int G = rle_load_objs(o, hdr, n);
    if ((long)blockIdx.x * RLE_PER_BLOCK >= G) return;
    const long g0 = (long)blockIdx.x * RLE_PER_BLOCK + threadIdx.x * 4;
    int val[4], nch[4], sum = 0;
    for (int q = 0; q < 4; ++q) {
        const long g = g0 + q;
        nch[q] = 0;
        val[q] = 0;
        if (g < G) {
            int k, j, count;
            rle_value(o, B, n, (int)g, k, j, count, val[q]);
            if (count >= 0) nch[q] = rle_nchars(val[q]);
        }
        sum += nch[q];
    }
    int total;
    int at = blocksum[blockIdx.x] + rle_scan256(sum, o.red, total);
    for (int q = 0; q < 4; ++q) {
        int x = val[q];
        for (int i = 0; i < nch[q]; ++i, ++at) {
            int c = x & 0x1f;
            x >>= 5;
            if (i + 1 < nch[q]) c |= 0x20;
            if (at < cap) out[at] = (uint8_t)(c + 48);
        }
    }
}

// PROB_TO_ID flags == 32.  p2 = ids u8 [H, W], p3 = stream, i7 = capacity, p4 = status int32 [4], p5 = scratch int32 [i8], p6 = object ids
// int32 [i9], p7 = table int32 [i9, 4]
int launch_rle_encode(const cutie_op* op, hipStream_t s) {
    const uint64_t* p = op->p;
    const int H = op->i[1], W = op->i[2], cap = op->i[7], n = op->i[9];
    if (H < 1 || W < 1) { cutie_set_error("rle encode: empty shape (H, W >= 1)"); return -2; }
    if ((long)H * W >= (1l << 31)) { cutie_set_error("rle encode: %d x %d exceeds 2^31 positions", H, W); return -2; }
    if (n < 0 || n > 255) { cutie_set_error("rle encode: %d objects, 0 <= n <= 255", n); return -2; }
    if (cap < 0) { cutie_set_error("rle encode: negative capacity"); return -2; }
    if (!p[2] || (!p[3] && cap > 0) || !p[4] || !p[5] || (n > 0 && (!p[6] || !p[7]))) {
        cutie_set_error("rle encode: needs the id plane (p2), the stream (p3), the status (p4), the scratch (p5), the object ids (p6) and the table (p7)");
        return -2;
    }
    if ((p[4] & 3) || (p[5] & 15) || (p[6] & 3) || (p[7] & 15)) {
        cutie_set_error("rle encode: status and object ids 4-byte aligned, scratch and table 16-byte aligned");
        return -2;
    }
    const long HW = (long)H * W;
    const int nseg = (H + RLE_SEG - 1) / RLE_SEG;
    const long nchunk = (long)W * nseg, G = 2 * HW + n, nblk = rle_nblk(HW, n);
    const long need = RLE_HDR + ((nblk + 3) & ~3l) + n * nchunk + G;
    if ((long)op->i[8] < need) { cutie_set_error("rle encode: scratch of %d words, needs %ld", op->i[8], need); return -2; }
    int* hdr = (int*)p[5];
    int* blocksum = hdr + RLE_HDR;
    int* cnt = blocksum + ((nblk + 3) & ~3l);
    int* B = cnt + n * nchunk;
    if (n > 0) {
        const int tiles = ((W + RLE_TC - 1) / RLE_TC) * nseg;
        hipLaunchKernelGGL(rle_sweep_kernel<false>, dim3(tiles), dim3(256), 0, s, (const uint8_t*)p[2], H, W, (const int*)p[6], n, nseg, cnt, hdr, B, (int)G);
        hipLaunchKernelGGL(rle_chunkscan_kernel, dim3(n), dim3(256), 0, s, cnt, nchunk, hdr);
        hipLaunchKernelGGL(rle_sweep_kernel<true>, dim3(tiles), dim3(256), 0, s, (const uint8_t*)p[2], H, W, (const int*)p[6], n, nseg, cnt, hdr, B, (int)G);
        hipLaunchKernelGGL(rle_len_kernel, dim3((unsigned)nblk), dim3(256), 0, s, (const int*)B, hdr, n, blocksum);
    }
    hipLaunchKernelGGL(rle_finish_kernel, dim3(1), dim3(256), 0, s, (const int*)B, hdr, n, (int)HW, blocksum, (int4*)p[7], (int*)p[4], cap);
    if (n > 0)
        hipLaunchKernelGGL(rle_emit_kernel, dim3((unsigned)nblk), dim3(256), 0, s, (const int*)B, (const int*)hdr, n, (const int*)blocksum, (const int*)p[4],
                           (uint8_t*)p[3], cap);
    return (int)hipGetLastError();
}
