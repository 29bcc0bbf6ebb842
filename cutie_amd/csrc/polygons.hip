// PROB_TO_ID flags == 8192 (ABI 11, form added): the outlines of the listed objects of a uint8 id plane [H, W] as exact rings of lattice
// corners (slots, conventions and the definition of a ring: include/cutie_hip.h; the model: tests/polygon_ref.py).
//
// A directed boundary edge is named e = (tail vertex) * 4 + d.  Every lattice vertex sees the four pixels around it (NW NE / SW SE; outside
// the frame = the value 256, which is no id), and of the four edges that can leave it
//   d = 0 (E) exists iff SE is listed and SE != NE,      d = 1 (S) iff SW is listed and SW != SE,
//   d = 2 (W) iff NW is listed and NW != SW,             d = 3 (N) iff NE is listed and NE != NW        (the object lies on the right).
// SLOTS: the edges are compacted in the order of e (a block scan per 1024 vertices behind a scan of the block totals), so the smallest
// slot of a ring is its first edge and nothing below depends on an arrival order.  vbase[vertex] = the slot of the vertex's first edge; the
// slot of edge (v, d) is vbase[v] + popcount(mask(v) below d), and whoever asks has the four pixels of v in hand.
// The launches (kernel boundaries are the only ordering between blocks; no spin, no grid barrier):
//   1  ply_count_kernel     per block of 1024 vertices the number of edges
//   2  ply_scan_kernel      one block: exclusive scan of the block totals; E -> header and status word 3; E > E_cap sets the skip word, the
//                           error bit and a zero table, and every later kernel returns at once; clears the round flags
//   3  ply_emit_kernel      vbase[v], eid[slot]
//   4  ply_link_kernel      per slot: the successor by the rule of the connectivity (the first existing edge of the object at the head
//                           vertex in the order left, straight, right for 8 and right, straight, left for 4); it writes into the
//                           SUCCESSOR's word its predecessor and whether that successor is a corner (the direction changed); the object row
//   5  ply_round_kernel x ceil(log2 E_cap)   pointer jumping BACKWARDS.  The state of a slot after r rounds describes the window of 2^r
//                           edges i, pred(i), pred^2(i) ...: j = where the next window starts, m = the smallest slot in the window, d = how
//                           many steps back it lies (the nearest one, when the window wraps the ring), c = the corners among the first d
//                           edges of the window, t = the corners of the whole window.  Two windows combine associatively; when 2^r >= L,
//                           m is the ring's first edge, d the edge's rank in the ring and c, for a corner, its index among the ring's
//                           vertices.  The states are double-buffered (round r reads buffer r & 1 and writes the other).  A round in
//                           which no m fell leaves its flag 0, and the rounds behind it return at once: windows that tile a ring cannot
//                           all keep their minimum unless all hold the ring's.
//   (ply_small_kernel       i6 == 0 and E <= PLY_SMALL: one block does 5 .. 9 in LDS, see there; the launches below then return at once)
//   6  ply_heads_kernel     ring heads (d == 0) per block of 256 slots and object row: their number and their vertices
//   7  ply_offsets_kernel   one block: per row the scan over the blocks, then over the rows: the object table, R, V, the capacity check
//   8  ply_rings_kernel     ring rows into the stream (rank inside the block among the same row's earlier heads), each head's vertex offset
//   9  ply_verts_kernel     every corner writes x | y << 16 at its ring's offset + c
// Integers only; the only atomics are LDS minima / sums and an OR into a round flag, whose results do not depend on arrival order.
#include "common.h"

#define PLY_T 256                        // threads per block
#define PLY_VPB 1024                     // vertices per block of the count / emit sweeps
#define PLY_MAX_GRID 4096                // blocks of the per-slot sweeps (grid-stride beyond)
#define PLY_HDR 64                       // header words: 0 E | 1 skip | 2 the stream fits | 3 R | 16 .. 47 round flags
#define PLY_ABSENT 0x7fffffff
#define PLY_OUT 256                      // "id" of a pixel outside the frame

struct PlyScratch {                      // word offsets into p5, all multiples of 4 (OpList.polygon_scratch_words)
    long bsum, vbase, eid, orow, pred, st0, st1, t0, t1, hoff, bhr, bhv, row0, total;
};

__host__ __device__ static inline long ply_up4(long v) { return (v + 3) & ~3l; }

static PlyScratch ply_layout(long NV, long C) {
    PlyScratch L;
    const long nbv = (NV + PLY_VPB - 1) / PLY_VPB, nbs = (C + PLY_T - 1) / PLY_T;
    long o = PLY_HDR;
    L.bsum = o; o += ply_up4(nbv);
    L.vbase = o; o += ply_up4(NV);
    L.eid = o; o += ply_up4(C);
    L.orow = o; o += ply_up4(C);
    L.pred = o; o += ply_up4(C);
    L.st0 = o; o += 4 * ply_up4(C);
    L.st1 = o; o += 4 * ply_up4(C);
    L.t0 = o; o += ply_up4(C);
    L.t1 = o; o += ply_up4(C);
    L.hoff = o; o += ply_up4(C);
    L.bhr = o; o += 256 * nbs;
    L.bhv = o; o += 256 * nbs;
    L.row0 = o; o += 512;
    L.total = o;
    return L;
}

// id -> object row (the first entry that names it; entries outside 1 .. 255 name nothing), PLY_ABSENT where not listed; [256] = outside
__device__ __forceinline__ void ply_lut(int* s_lut, const int* __restrict__ objs, int n) {
    for (int k = threadIdx.x; k < 257; k += blockDim.x) s_lut[k] = PLY_ABSENT;
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        const int id = objs[k];
        if (id >= 1 && id <= 255) atomicMin(&s_lut[id], k);
    }
    __syncthreads();
}

__device__ __forceinline__ int ply_px(const uint8_t* __restrict__ ids, int H, int W, int x, int y) {
    return (x >= 0 && y >= 0 && x < W && y < H) ? (int)ids[(long)y * W + x] : PLY_OUT;
}

// the four pixels around vertex (x, y): q[0] NW, q[1] NE, q[2] SW, q[3] SE
__device__ __forceinline__ void ply_quad(const uint8_t* __restrict__ ids, int H, int W, int x, int y, int* q) {
    q[0] = ply_px(ids, H, W, x - 1, y - 1);
    q[1] = ply_px(ids, H, W, x, y - 1);
    q[2] = ply_px(ids, H, W, x - 1, y);
    q[3] = ply_px(ids, H, W, x, y);
}

// per direction d: the pixel of the object (on the right) and the pixel across, as indices into the quad of the TAIL vertex
__device__ __forceinline__ int ply_in(int d) { return (0x1023 >> (4 * d)) & 3; }       // d 0 -> 3 (SE), 1 -> 2 (SW), 2 -> 0 (NW), 3 -> 1 (NE)
__device__ __forceinline__ int ply_across(int d) { return (0x0231 >> (4 * d)) & 3; }   // d 0 -> 1 (NE), 1 -> 3 (SE), 2 -> 2 (SW), 3 -> 0 (NW)

__device__ __forceinline__ unsigned ply_mask(const int* q, const int* s_lut) {
    unsigned m = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int a = q[ply_in(d)], b = q[ply_across(d)];
        m |= (s_lut[a] != PLY_ABSENT && a != b) ? 1u << d : 0u;
    }
    return m;
}

// exclusive scan of v over the block's 64 * WAVES threads; *total = the block's sum.  s_w: WAVES words of LDS
template <int WAVES = PLY_T / 64>
__device__ __forceinline__ int ply_block_scan(int v, int* s_w, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    __syncthreads();                                           // (the previous use of s_w is over)
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int t = s_w[w];
        base += w < wave ? t : 0;
        sum += t;
    }
    *total = sum;
    return base + inc - v;
}

template <bool EMIT>
__global__ __launch_bounds__(PLY_T) void ply_sweep_kernel(const uint8_t* __restrict__ ids, const int* __restrict__ objs, int n, int H, int W, long NV,
                                                          int* __restrict__ hdr, int* __restrict__ bsum, int* __restrict__ vbase, int* __restrict__ eid) {
    __shared__ int s_lut[257];
    __shared__ int s_w[8];
    if (EMIT && hdr[1]) return;
    ply_lut(s_lut, objs, n);
    const int E = EMIT ? hdr[0] : 0;
    int carry = EMIT ? bsum[blockIdx.x] : 0;
    for (int k = 0; k < PLY_VPB / PLY_T; ++k) {
        const long v = (long)blockIdx.x * PLY_VPB + k * PLY_T + threadIdx.x;
        unsigned m = 0;
        if (v < NV) {
            int q[4];
            ply_quad(ids, H, W, (int)(v % (W + 1)), (int)(v / (W + 1)), q);
            m = ply_mask(q, s_lut);
        }
        int total;
        const int at = carry + ply_block_scan(__popc(m), s_w, &total);
        carry += total;
        if (EMIT && v < NV) {
            vbase[v] = at;
            int s = at;
            for (int d = 0; d < 4; ++d)
                if (m >> d & 1) {
                    if (s < E) eid[s] = (int)(v * 4 + d);      // (s < E by construction; the guard keeps a mistake inside the scratch)
                    ++s;
                }
        }
    }
    if (!EMIT && threadIdx.x == 0) bsum[blockIdx.x] = carry;
}

__global__ __launch_bounds__(PLY_T) void ply_scan_kernel(int* __restrict__ hdr, int* __restrict__ bsum, long nbv, int C, int n, int* __restrict__ status,
                                                         int* __restrict__ table) {
    __shared__ int s_w[8];
    int carry = 0;
    for (long b0 = 0; b0 < nbv; b0 += PLY_T) {
        const long b = b0 + threadIdx.x;
        const int v = b < nbv ? bsum[b] : 0;
        int total;
        const int at = carry + ply_block_scan(v, s_w, &total);
        if (b < nbv) bsum[b] = at;
        carry += total;
    }
    const int E = carry, skip = E > C;
    if (threadIdx.x < 32) hdr[16 + threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        hdr[0] = E;
        hdr[1] = skip;
        hdr[2] = 0;
        hdr[3] = 0;
        status[3] = E;
        if (skip) { status[0] = 0; status[1] = 2; status[2] = 0; }
    }
    if (skip)
        for (int k = threadIdx.x; k < 4 * n; k += PLY_T) table[k] = 0;
}

__global__ __launch_bounds__(PLY_T) void ply_link_kernel(const uint8_t* __restrict__ ids, const int* __restrict__ objs, int n, int H, int W, int conn,
                                                         const int* __restrict__ hdr, const int* __restrict__ vbase, const int* __restrict__ eid,
                                                         int* __restrict__ orow, unsigned* __restrict__ pred) {
    __shared__ int s_lut[257];
    if (hdr[1]) return;
    const int E = hdr[0];
    if ((long)blockIdx.x * PLY_T >= E) return;
    ply_lut(s_lut, objs, n);
    for (long i = (long)blockIdx.x * PLY_T + threadIdx.x; i < E; i += (long)gridDim.x * PLY_T) {
        const int e = eid[i], d = e & 3, v = e >> 2, x = v % (W + 1), y = v / (W + 1);
        int q[4];
        ply_quad(ids, H, W, x, y, q);
        const int val = q[ply_in(d)];
        orow[i] = s_lut[val];
        const int hx = x + (d == 0) - (d == 2), hy = y + (d == 1) - (d == 3);
        ply_quad(ids, H, W, hx, hy, q);
        const int first = conn == 8 ? 3 : 1, step = conn == 8 ? 1 : 3;     // 8: left, straight, right; 4: right, straight, left
        int nd = -1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int c = (d + first + k * step) & 3;
            if (nd < 0 && q[ply_in(c)] == val && q[ply_across(c)] != val) nd = c;
        }
        if (nd < 0) continue;                                  // (cannot happen: an edge that arrives has one that leaves)
        const unsigned m = ply_mask(q, s_lut);
        const long hv = (long)hy * (W + 1) + hx;
        const int s = vbase[hv] + __popc(m & ((1u << nd) - 1u));
        if (s >= 0 && s < E) pred[s] = (unsigned)i | (nd != d ? 0x80000000u : 0u);
    }
}

struct PlyState { unsigned j, m, d, c, t; };

// the state of slot i after r rounds: synthesised from pred[] for r == 0, else from buffer r & 1.  Indices are clamped below E: a mistake
// upstream cannot leave the scratch.
__device__ __forceinline__ PlyState ply_load(int r, unsigned i, int E, const unsigned* __restrict__ pred, const uint4* __restrict__ st0,
                                             const uint4* __restrict__ st1, const unsigned* __restrict__ t0, const unsigned* __restrict__ t1) {
    PlyState s;
    i = min(i, (unsigned)(E - 1));
    if (r == 0) {
        const unsigned p = pred[i];
        s.j = min(p & 0x7fffffffu, (unsigned)(E - 1)); s.m = i; s.d = 0; s.c = 0; s.t = p >> 31;
    } else {
        const uint4 q = (r & 1) ? st1[i] : st0[i];
        s.j = min(q.x, (unsigned)(E - 1)); s.m = q.y; s.d = q.z; s.c = q.w; s.t = (r & 1) ? t1[i] : t0[i];
    }
    return s;
}

// rounds that ran: round 0 always, round r iff round r - 1 lowered a minimum (flags are a prefix of ones)
__device__ __forceinline__ int ply_rounds_done(const int* hdr, int NR) {
    int r = 0;
    while (r < NR && (r == 0 || hdr[16 + r - 1] != 0)) ++r;
    return r;
}

__global__ __launch_bounds__(PLY_T) void ply_round_kernel(int r, int* __restrict__ hdr, const unsigned* __restrict__ pred, uint4* __restrict__ st0,
                                                          uint4* __restrict__ st1, unsigned* __restrict__ t0, unsigned* __restrict__ t1) {
    if (hdr[1] || (r > 0 && hdr[16 + r - 1] == 0)) return;
    const int E = hdr[0];
    bool changed = false;
    for (long i = (long)blockIdx.x * PLY_T + threadIdx.x; i < E; i += (long)gridDim.x * PLY_T) {
        const PlyState a = ply_load(r, (unsigned)i, E, pred, st0, st1, t0, t1);
        const PlyState b = ply_load(r, a.j, E, pred, st0, st1, t0, t1);
        uint4 o;
        o.x = b.j;
        if (b.m < a.m) { o.y = b.m; o.z = (1u << r) + b.d; o.w = a.t + b.c; changed = true; }
        else { o.y = a.m; o.z = a.d; o.w = a.c; }
        if (r & 1) { st0[i] = o; t0[i] = a.t + b.t; }
        else { st1[i] = o; t1[i] = a.t + b.t; }
    }
    if (__any(changed) && (threadIdx.x & 63) == 0) atomicOr(&hdr[16 + r], 1);
}

// a ring head's row, vertices and edges (h: its state; the last edge of the ring is its predecessor)
#define PLY_FINAL_ARGS const int* __restrict__ hdr, int NR, const unsigned* __restrict__ pred, const uint4* __restrict__ st0, const uint4* __restrict__ st1, \
                       const unsigned* __restrict__ t0, const unsigned* __restrict__ t1

__global__ __launch_bounds__(PLY_T) void ply_heads_kernel(PLY_FINAL_ARGS, const int* __restrict__ orow, int* __restrict__ bhr, int* __restrict__ bhv) {
    __shared__ int s_r[256], s_v[256];
    if (hdr[1]) return;
    const int E = hdr[0], X = ply_rounds_done(hdr, NR);
    const long nbs = ((long)E + PLY_T - 1) / PLY_T;
    for (long b = blockIdx.x; b < nbs; b += gridDim.x) {
        s_r[threadIdx.x] = 0;
        s_v[threadIdx.x] = 0;
        __syncthreads();
        const long i = b * PLY_T + threadIdx.x;
        if (i < E) {
            const PlyState h = ply_load(X, (unsigned)i, E, pred, st0, st1, t0, t1);
            if (h.d == 0) {
                const PlyState l = ply_load(X, pred[i] & 0x7fffffffu, E, pred, st0, st1, t0, t1);
                const int k = orow[i] & 255;
                atomicAdd(&s_r[k], 1);
                atomicAdd(&s_v[k], (int)l.c + 1);
            }
        }
        __syncthreads();
        bhr[b * 256 + threadIdx.x] = s_r[threadIdx.x];
        bhv[b * 256 + threadIdx.x] = s_v[threadIdx.x];
        __syncthreads();
    }
}

__global__ __launch_bounds__(PLY_T) void ply_offsets_kernel(int* __restrict__ hdr, int n, int cap_bytes, int* __restrict__ bhr, int* __restrict__ bhv,
                                                            int* __restrict__ row0, int* __restrict__ status, int* __restrict__ table) {
    __shared__ int s_r[256], s_v[256], s_r0[256], s_v0[256], s_fit;
    if (hdr[1]) return;
    const int E = hdr[0], k = threadIdx.x;
    const long nbs = ((long)E + PLY_T - 1) / PLY_T;
    int r = 0, v = 0;
    for (long b = 0; b < nbs; ++b) {                           // exclusive scan over the blocks, per row (E comes from an earlier launch)
        const int cr = bhr[b * 256 + k], cv = bhv[b * 256 + k];
        bhr[b * 256 + k] = r;
        bhv[b * 256 + k] = v;
        r += cr;
        v += cv;
    }
    s_r[k] = r;
    s_v[k] = v;
    __syncthreads();
    if (k == 0) {
        int R = 0, V = 0;
        for (int q = 0; q < n; ++q) { s_r0[q] = R; s_v0[q] = V; R += s_r[q]; V += s_v[q]; }
        const long bytes = 16l * R + 4l * V;
        const int fit = bytes <= (long)cap_bytes;
        s_fit = fit;
        hdr[2] = fit;
        hdr[3] = R;
        status[0] = (int)(bytes > 0x7fffffffl ? 0x7fffffffl : bytes);
        status[1] = fit ? 0 : 1;
        status[2] = R;
        status[3] = E;
    }
    __syncthreads();
    if (k < n) {
        const int fit = s_fit;
        row0[k] = s_r0[k];
        row0[256 + k] = s_v0[k];
        table[4 * k + 0] = fit ? s_r0[k] : 0;
        table[4 * k + 1] = s_r[k];
        table[4 * k + 2] = fit ? s_v0[k] : 0;
        table[4 * k + 3] = s_v[k];
    }
}

__global__ __launch_bounds__(PLY_T) void ply_rings_kernel(PLY_FINAL_ARGS, const int* __restrict__ orow, const int* __restrict__ bhr, const int* __restrict__ bhv,
                                                          const int* __restrict__ row0, int* __restrict__ hoff, int* __restrict__ stream, long cap_words) {
    __shared__ int s_k[256], s_n[256];
    if (hdr[1] || !hdr[2]) return;
    const int E = hdr[0], X = ply_rounds_done(hdr, NR);
    const long nbs = ((long)E + PLY_T - 1) / PLY_T;
    for (long b = blockIdx.x; b < nbs; b += gridDim.x) {
        const long i = b * PLY_T + threadIdx.x;
        int k = -1, vn = 0, len = 0;
        if (i < E) {
            const PlyState h = ply_load(X, (unsigned)i, E, pred, st0, st1, t0, t1);
            if (h.d == 0) {
                const PlyState l = ply_load(X, pred[i] & 0x7fffffffu, E, pred, st0, st1, t0, t1);
                k = orow[i] & 255;
                vn = (int)l.c + 1;
                len = (int)l.d + 1;
            }
        }
        s_k[threadIdx.x] = k;
        s_n[threadIdx.x] = vn;
        __syncthreads();
        if (k >= 0) {
            int ring = row0[k] + bhr[b * 256 + k], voff = row0[256 + k] + bhv[b * 256 + k];
            for (int q = 0; q < (int)threadIdx.x; ++q)          // the same row's heads in front of this one inside the block
                if (s_k[q] == k) { ++ring; voff += s_n[q]; }
            hoff[i] = voff;
            if (ring >= 0 && 4l * ring + 4 <= cap_words) {
                int4 row;
                row.x = k; row.y = voff; row.z = vn; row.w = len;
                ((int4*)stream)[ring] = row;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(PLY_T) void ply_verts_kernel(PLY_FINAL_ARGS, const int* __restrict__ eid, const int* __restrict__ hoff, int W,
                                                          unsigned* __restrict__ stream, long cap_words) {
    if (hdr[1] || !hdr[2]) return;
    const int E = hdr[0], X = ply_rounds_done(hdr, NR);
    const long R = hdr[3];
    for (long i = (long)blockIdx.x * PLY_T + threadIdx.x; i < E; i += (long)gridDim.x * PLY_T) {
        if (!(pred[i] >> 31)) continue;
        const PlyState s = ply_load(X, (unsigned)i, E, pred, st0, st1, t0, t1);
        const long at = 4 * R + (long)hoff[min(s.m, (unsigned)(E - 1))] + (long)s.c;
        const int v = eid[i] >> 2, x = v % (W + 1), y = v / (W + 1);
        if (at >= 4 * R && at < cap_words) stream[at] = (unsigned)x | (unsigned)y << 16;
    }
}

// THE SMALL PATH: E <= PLY_SMALL edges fit one workgroup's LDS (12 bytes per edge: j | m << 16, d | c << 16, t | pred << 16 with the corner
// bit on top; 48 KiB, and 10 KiB of ring heads and row sums), so one block of 1024 threads runs the rounds between __syncthreads(), as many
// as E needs, then the ring order, the offsets and the scatter.  The converged m, d and c are those of the general path, and so is every
// word written.  It ends by setting the skip word: the launches of the general path behind it return at once.
#define PLY_SMALL 4096
#define PLY_ST 1024
#define PLY_SPT (PLY_SMALL / PLY_ST)

__global__ __launch_bounds__(PLY_ST) void ply_small_kernel(int* __restrict__ hdr, int n, int cap_bytes, int W, const unsigned* __restrict__ pred,
                                                           const int* __restrict__ orow, const int* __restrict__ eid, int* __restrict__ hoff,
                                                           int* __restrict__ status, int* __restrict__ table, int* __restrict__ stream) {
    __shared__ unsigned s_a[PLY_SMALL], s_b[PLY_SMALL], s_c[PLY_SMALL];      // j | m << 16;  d | c << 16;  t | pred << 16 | corner << 31
    __shared__ int s_key[PLY_SMALL / 4];                                     // ring heads in slot order: slot | row << 12
    __shared__ unsigned short s_vn[PLY_SMALL / 4], s_len[PLY_SMALL / 4];
    __shared__ int s_rr[256], s_rv[256], s_r0[256], s_v0[256], s_w[PLY_ST / 64], s_fit;
    if (hdr[1]) return;
    const int E = hdr[0], tid = threadIdx.x;
    if (E > PLY_SMALL) return;
    for (int k = 0; k < PLY_SPT; ++k) {
        const int i = tid + k * PLY_ST;
        if (i < E) {
            const unsigned p = pred[i], j = min(p & 0x7fffffffu, (unsigned)(E - 1));
            s_a[i] = j | (unsigned)i << 16;
            s_b[i] = 0;
            s_c[i] = (p >> 31) | j << 16 | (p & 0x80000000u);
        }
    }
    if (tid < 256) { s_rr[tid] = 0; s_rv[tid] = 0; }
    __syncthreads();
    for (int r = 0; (1 << r) < E; ++r) {                       // (E comes from an earlier launch; the whole block takes the same trips)
        unsigned na[PLY_SPT], nb[PLY_SPT], nt[PLY_SPT];
        for (int k = 0; k < PLY_SPT; ++k) {
            const int i = tid + k * PLY_ST;
            if (i < E) {
                const unsigned a = s_a[i], j = a & 0xffffu, b = s_a[j];
                const unsigned ta = s_c[i] & 0xffffu, tb = s_c[j] & 0xffffu;
                nt[k] = (ta + tb) & 0xffffu;
                if ((b >> 16) < (a >> 16)) {
                    const unsigned db = s_b[j];
                    na[k] = (b & 0xffffu) | (b & 0xffff0000u);
                    nb[k] = (((1u << r) + (db & 0xffffu)) & 0xffffu) | ((ta + (db >> 16)) & 0xffffu) << 16;
                } else {
                    na[k] = (b & 0xffffu) | (a & 0xffff0000u);
                    nb[k] = s_b[i];
                }
            }
        }
        __syncthreads();
        for (int k = 0; k < PLY_SPT; ++k) {
            const int i = tid + k * PLY_ST;
            if (i < E) { s_a[i] = na[k]; s_b[i] = nb[k]; s_c[i] = (s_c[i] & 0xffff0000u) | nt[k]; }
        }
        __syncthreads();
    }
    // the ring heads in slot order
    int carry = 0;
    for (int k = 0; k < PLY_SPT; ++k) {
        const int i = tid + k * PLY_ST;
        const bool head = i < E && (s_b[i] & 0xffffu) == 0;
        int total;
        const int at = carry + ply_block_scan<PLY_ST / 64>(head ? 1 : 0, s_w, &total);
        carry += total;
        if (head && at < PLY_SMALL / 4) {
            const unsigned l = s_b[(s_c[i] >> 16) & 0x7fffu];            // the ring's last edge
            const int row = orow[i] & 255, vn = (int)(l >> 16) + 1;
            s_key[at] = i | row << 12;
            s_vn[at] = (unsigned short)vn;
            s_len[at] = (unsigned short)((l & 0xffffu) + 1);
            atomicAdd(&s_rr[row], 1);
            atomicAdd(&s_rv[row], vn);
        }
    }
    const int R = min(carry, PLY_SMALL / 4);
    __syncthreads();
    if (tid == 0) {
        int r = 0, v = 0;
        for (int q = 0; q < n; ++q) { s_r0[q] = r; s_v0[q] = v; r += s_rr[q]; v += s_rv[q]; }
        const int bytes = 16 * r + 4 * v, fit = bytes <= cap_bytes;
        s_fit = fit;
        status[0] = bytes;
        status[1] = fit ? 0 : 1;
        status[2] = r;
        status[3] = E;
    }
    __syncthreads();
    const int fit = s_fit;
    if (tid < n) {
        table[4 * tid + 0] = fit ? s_r0[tid] : 0;
        table[4 * tid + 1] = s_rr[tid];
        table[4 * tid + 2] = fit ? s_v0[tid] : 0;
        table[4 * tid + 3] = s_rv[tid];
    }
    if (fit) {
        const long cap_words = cap_bytes / 4;
        for (int h = tid; h < R; h += PLY_ST) {
            const int key = s_key[h], row = key >> 12;
            int ring = s_r0[row], voff = s_v0[row];
            for (int q = 0; q < h; ++q)                       // the same row's heads in front of this one
                if ((s_key[q] >> 12) == row) { ++ring; voff += s_vn[q]; }
            hoff[key & 0xfff] = voff;
            if (4l * ring + 4 <= cap_words) {
                int4 out;
                out.x = row; out.y = voff; out.z = s_vn[h]; out.w = s_len[h];
                ((int4*)stream)[ring] = out;
            }
        }
        __syncthreads();                                       // (hoff: written and read by this block alone)
        for (int k = 0; k < PLY_SPT; ++k) {
            const int i = tid + k * PLY_ST;
            if (i < E && (s_c[i] >> 31)) {
                const long at = 4l * R + hoff[(s_a[i] >> 16) & 0xfffu] + (long)(s_b[i] >> 16);
                const int v = eid[i] >> 2;
                if (at < cap_words) ((unsigned*)stream)[at] = (unsigned)(v % (W + 1)) | (unsigned)(v / (W + 1)) << 16;
            }
        }
    }
    __syncthreads();
    if (tid == 0) hdr[1] = 1;                                  // done: the general path's launches return at once
}

__global__ void ply_empty_kernel(int* __restrict__ status) {
    if (threadIdx.x < 4) status[threadIdx.x] = 0;
}

// words of scratch for a plane of H x W and E_cap edges: OpList.polygon_scratch_words states the same sum
static long ply_scratch_words(int H, int W, long C) { return ply_layout((long)(H + 1) * (W + 1), C).total; }

// PROB_TO_ID flags == 8192.  p2 = ids u8 [i1, i2], read only; p6 = object ids int32 [i9]; i5 = connectivity; i6 = path; i3 = E_cap;
// p5 = scratch int32 [i8 + 2^31 i7]; p3 = stream of i4 bytes; p7 = table int32 [i9, 4]; p4 = status int32 [4]
int launch_polygon_trace(const cutie_op* op, hipStream_t s) {
    const uint64_t* p = op->p;
    const int H = op->i[1], W = op->i[2], C = op->i[3], cap = op->i[4], conn = op->i[5], path = op->i[6], n = op->i[9];
    if (H < 1 || W < 1) { cutie_set_error("polygon trace: empty shape (H, W >= 1)"); return -2; }
    if (H > 65535 || W > 65535) { cutie_set_error("polygon trace: %d x %d, a vertex packs x and y into 16 bits each (H, W <= 65535)", H, W); return -2; }
    const long NV = (long)(H + 1) * (W + 1);
    if (NV >= (1l << 29)) { cutie_set_error("polygon trace: %d x %d has 2^29 lattice vertices or more (the edge index has 31 bits)", H, W); return -2; }
    if (n < 0 || n > 255) { cutie_set_error("polygon trace: %d objects, 0 <= n <= 255", n); return -2; }
    if (conn != 4 && conn != 8) { cutie_set_error("polygon trace: connectivity %d, 4 or 8", conn); return -2; }
    if (path < 0 || path > 1) { cutie_set_error("polygon trace: path %d, 0 (the launcher chooses) or 1 (the general path)", path); return -2; }
    if (C < 1) { cutie_set_error("polygon trace: edge capacity %d, E_cap >= 1", C); return -2; }
    if (cap < 0 || (cap & 3)) { cutie_set_error("polygon trace: stream capacity %d, not negative and a multiple of 4", cap); return -2; }
    if (!p[2]) { cutie_set_error("polygon trace: needs the id plane (p2)"); return -2; }
    if (!p[4]) { cutie_set_error("polygon trace: needs the status (p4)"); return -2; }
    if (p[4] & 3) { cutie_set_error("polygon trace: status 4-byte aligned"); return -2; }
    if (!p[3] && cap > 0) { cutie_set_error("polygon trace: needs the stream (p3)"); return -2; }      // (a stream of no bytes may be null)
    if (p[3] & 15) { cutie_set_error("polygon trace: stream 16-byte aligned"); return -2; }
    if (!p[5]) { cutie_set_error("polygon trace: needs the scratch (p5)"); return -2; }
    if (p[5] & 15) { cutie_set_error("polygon trace: scratch 16-byte aligned"); return -2; }
    if (n > 0 && !p[6]) { cutie_set_error("polygon trace: needs the object ids (p6)"); return -2; }
    if (p[6] & 3) { cutie_set_error("polygon trace: object ids 4-byte aligned"); return -2; }
    if (n > 0 && !p[7]) { cutie_set_error("polygon trace: needs the object table (p7)"); return -2; }
    if (p[7] & 15) { cutie_set_error("polygon trace: object table 16-byte aligned"); return -2; }
    const long need = ply_scratch_words(H, W, C);
    const long words = (op->i[8] < 0 || op->i[7] < 0) ? -1l : (long)op->i[8] + ((long)op->i[7] << 31);
    if (words < need) { cutie_set_error("polygon trace: scratch of %ld words, %d x %d with %d edges need %ld", words, H, W, C, need); return -2; }
    int* status = (int*)p[4];
    if (n == 0) {
        hipLaunchKernelGGL(ply_empty_kernel, dim3(1), dim3(64), 0, s, status);
        return (int)hipGetLastError();
    }
    const PlyScratch L = ply_layout(NV, C);
    int* w = (int*)p[5];
    int *hdr = w, *bsum = w + L.bsum, *vbase = w + L.vbase, *eid = w + L.eid, *orow = w + L.orow, *hoff = w + L.hoff, *bhr = w + L.bhr, *bhv = w + L.bhv,
        *row0 = w + L.row0, *table = (int*)p[7];
    unsigned *pred = (unsigned*)(w + L.pred), *t0 = (unsigned*)(w + L.t0), *t1 = (unsigned*)(w + L.t1);
    uint4 *st0 = (uint4*)(w + L.st0), *st1 = (uint4*)(w + L.st1);
    const uint8_t* ids = (const uint8_t*)p[2];
    const int* objs = (const int*)p[6];
    const long nbv = (NV + PLY_VPB - 1) / PLY_VPB;
    long gs = ((long)C + PLY_T - 1) / PLY_T;
    if (gs > PLY_MAX_GRID) gs = PLY_MAX_GRID;
    int NR = 0;
    while ((1l << NR) < (long)C) ++NR;                         // <= 31: after NR rounds a window holds 2^NR >= E_cap >= L edges
    const dim3 T(PLY_T), G((unsigned)gs);
    hipLaunchKernelGGL(ply_sweep_kernel<false>, dim3((unsigned)nbv), T, 0, s, ids, objs, n, H, W, NV, hdr, bsum, vbase, eid);
    hipLaunchKernelGGL(ply_scan_kernel, dim3(1), T, 0, s, hdr, bsum, nbv, C, n, status, table);
    hipLaunchKernelGGL(ply_sweep_kernel<true>, dim3((unsigned)nbv), T, 0, s, ids, objs, n, H, W, NV, hdr, bsum, vbase, eid);
    hipLaunchKernelGGL(ply_link_kernel, G, T, 0, s, ids, objs, n, H, W, conn, (const int*)hdr, (const int*)vbase, (const int*)eid, orow, pred);
    if (path == 0)
        hipLaunchKernelGGL(ply_small_kernel, dim3(1), dim3(PLY_ST), 0, s, hdr, n, cap, W, (const unsigned*)pred, (const int*)orow, (const int*)eid, hoff,
                           status, table, (int*)p[3]);
    for (int r = 0; r < NR; ++r) hipLaunchKernelGGL(ply_round_kernel, G, T, 0, s, r, hdr, (const unsigned*)pred, st0, st1, t0, t1);
    hipLaunchKernelGGL(ply_heads_kernel, G, T, 0, s, (const int*)hdr, NR, (const unsigned*)pred, (const uint4*)st0, (const uint4*)st1, (const unsigned*)t0,
                       (const unsigned*)t1, (const int*)orow, bhr, bhv);
    hipLaunchKernelGGL(ply_offsets_kernel, dim3(1), T, 0, s, hdr, n, cap, bhr, bhv, row0, status, table);
    hipLaunchKernelGGL(ply_rings_kernel, G, T, 0, s, (const int*)hdr, NR, (const unsigned*)pred, (const uint4*)st0, (const uint4*)st1, (const unsigned*)t0,
                       (const unsigned*)t1, (const int*)orow, (const int*)bhr, (const int*)bhv, (const int*)row0, hoff, (int*)p[3], (long)cap / 4);
    hipLaunchKernelGGL(ply_verts_kernel, G, T, 0, s, (const int*)hdr, NR, (const unsigned*)pred, (const uint4*)st0, (const uint4*)st1, (const unsigned*)t0,
                       (const unsigned*)t1, (const int*)eid, (const int*)hoff, W, (unsigned*)p[3], (long)cap / 4);
    return (int)hipGetLastError();
}
