// PROB_TO_ID flags == 2048 (ABI 11, form added): connected components of a uint8 id plane [H, W], and the two clean-ups every consumer of
// segmentation masks runs on them -- object components below min_region pixels become background (stage A, islands), enclosed background
// components below fill_holes pixels become the object left of their first pixel (stage B, holes, on A's result).  The plane is rewritten
// in place (slots and conventions: include/cutie_hip.h; the numpy model: tests/region_ref.py).
//
// A stage is four launches over two int32 arrays of H W words in the scratch, label[] and size[]:
//   1  rgn_local_kernel   one block per tile of RGN_TH x RGN_TW pixels, ids and labels in LDS.  A wave owns a row: one ballot gives every
//                         pixel the start of its row run.  Runs are united with the row above (x; x - 1 and x + 1 as well under
//                         8-connectivity) by atomicMin union-find in LDS, then flattened.  label[p] = the global linear index of p's local
//                         root; size[local root] = area of the local component | its touches-the-frame-border bit (bit 31), 0 elsewhere.
//                         No global atomics.
//   2  rgn_seam_kernel    one thread per pixel of a tile's top row and left column: union with the neighbours across the seam (the diagonal
//                         ones and the tile corners under 8-connectivity).  label[] is written by other blocks, on other XCDs, in this
//                         launch: EVERY read of a label here is a relaxed agent-scope atomic load (it bypasses the CU's L1, which no other
//                         CU's store refreshes) and every write is an atomicMin on the larger root.  Lock-free: a thread retries while the
//                         two roots differ; nothing waits for another block -- no flags, tickets or spins.
//   3  rgn_size_kernel    one thread per local root (size != 0): it finds the global root and, if that is another pixel, adds its area and
//                         ORs its border bit into the root's slot -- one integer atomic per (tile, component), not per pixel -- and points
//                         its own label at the root, so that launch 4 walks at most two links.  The slots that are added to belong to global
//                         roots, whose own threads do nothing; a label is only ever replaced by an ancestor of what it held, so a reader
//                         that sees the old value walks a longer, equally valid chain.
//   4  rgn_apply_kernel   every pixel of the stage's kind finds its root, reads area and bit and rewrites its byte; a block adds its
//                         partial counts to counts[] (only blocks that changed something issue an atomic).
// Links go from the larger linear index to the smaller (atomicMin), so a component's root is its smallest linear index -- its first pixel
// in raster order -- whatever the arrival order; areas and counts are integer sums: the plane and counts depend on the plane and the three
// parameters alone.  That property also makes the fill pixel of a hole root - 1.
// In place is race-free: in stage A a pixel's decision depends on label[] and size[] only, and a thread writes no byte but its own.  In
// stage B only zero pixels are rewritten, and the one other byte a thread reads, plane[root - 1], is not zero (if it were, it would belong
// to the component and precede its first pixel; root is not in column 0, or the component would touch the border) -- so no thread of the
// launch writes it.
#include "common.h"

#define RGN_TH 16                        // tile height: OpList.REGION_TILE_H
#define RGN_TW 64                        // tile width = one wave per row: OpList.REGION_TILE_W
#define RGN_BORDER 0x80000000u

// ---- LDS union-find (launch 1) -----------------------------------------------------------------------------------------------------------------
// (a relaxed workgroup-scope atomic load: re-read in every round, and still a ds_read -- a volatile pointer loses the LDS address space)
__device__ __forceinline__ int rgn_find_lds(int* lab, int a) {
    int p;
    while ((p = __hip_atomic_load(&lab[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != a) a = p;
    return a;
}

__device__ __forceinline__ void rgn_union_lds(int* lab, int a, int b) {
    for (;;) {
        a = rgn_find_lds(lab, a);
        b = rgn_find_lds(lab, b);
        if (a == b) return;
        if (a > b) { const int c = a; a = b; b = c; }
        const int old = atomicMin(&lab[b], a);                 // hang the larger root under the smaller
        if (old == b) return;
        b = old;                                               // b had been linked meanwhile: go on with what it pointed at
    }
}

// the stage's kind of pixel: its id as the key (equal keys connect), -1 for every other pixel
__device__ __forceinline__ int rgn_key(int v, int holes) { return (holes ? v == 0 : v != 0) ? v : -1; }

__global__ __launch_bounds__(256) void rgn_local_kernel(const uint8_t* __restrict__ ids, int H, int W, int tiles_x, int holes, int conn8,
                                                        int* __restrict__ label, unsigned* __restrict__ size, int* __restrict__ zero) {
    __shared__ short s_key[RGN_TH * RGN_TW];
    __shared__ int s_lab[RGN_TH * RGN_TW];
    __shared__ unsigned s_area[RGN_TH * RGN_TW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (zero && blockIdx.x == 0 && t < 4) zero[t] = 0;         // counts, WRITTEN by the first launch of the op
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
    const int y0 = ty * RGN_TH, x = tx * RGN_TW + lane;
    for (int r = wave; r < RGN_TH; r += 4) {
        const int y = y0 + r;
        int key = -1;
        if (y < H && x < W) key = rgn_key(ids[(long)y * W + x], holes);
        s_key[r * RGN_TW + lane] = (short)key;
        s_area[r * RGN_TW + lane] = 0u;
    }
    __syncthreads();
    // every pixel to the start of its row run (runs of -1 included: nobody reads their labels)
    for (int r = wave; r < RGN_TH; r += 4) {
        const int li = r * RGN_TW + lane;
        const bool same = lane > 0 && s_key[li] == s_key[li - 1];
        const unsigned long long starts = __ballot(!same);     // (bit 0 is always set)
        const unsigned long long upto = starts & ((2ull << lane) - 1ull);
        s_lab[li] = r * RGN_TW + 63 - __clzll((long long)upto);
    }
    __syncthreads();
    for (int r = wave; r < RGN_TH; r += 4) {
        if (r == 0) continue;
        const int li = r * RGN_TW + lane, up = li - RGN_TW, key = s_key[li];
        if (key < 0) continue;
        if (s_key[up] == key) {
            // (where the left neighbour is of my run and of the upper one's, its union is mine)
            if (!(lane > 0 && s_key[li - 1] == key && s_key[up - 1] == key)) rgn_union_lds(s_lab, li, up);
        } else if (conn8) {                                    // (with an equal pixel above, the diagonal ones are of its run)
            if (lane > 0 && s_key[up - 1] == key) rgn_union_lds(s_lab, li, up - 1);
            if (lane < 63 && s_key[up + 1] == key) rgn_union_lds(s_lab, li, up + 1);
        }
    }
    __syncthreads();
    for (int r = wave; r < RGN_TH; r += 4) {                   // flatten (a label is only replaced by an ancestor: readers may see either)
        const int li = r * RGN_TW + lane;
        if (s_key[li] >= 0) s_lab[li] = rgn_find_lds(s_lab, li);
    }
    __syncthreads();
    for (int r = wave; r < RGN_TH; r += 4) {                   // one LDS atomic per run: its length, and whether it touches the frame's border
        const int li = r * RGN_TW + lane, y = y0 + r, key = s_key[li];
        const bool same = lane > 0 && key == s_key[li - 1];
        const unsigned long long starts = __ballot(!same);
        if (same || key < 0) continue;
        const unsigned long long above = lane == 63 ? 0ull : starts & ~((2ull << lane) - 1ull);
        const int len = (above ? __ffsll((long long)above) - 1 : 64) - lane;
        const int root = s_lab[li];
        atomicAdd(&s_area[root], (unsigned)len);
        if (y == 0 || y == H - 1 || x == 0 || x + len - 1 == W - 1) atomicOr(&s_area[root], RGN_BORDER);
    }
    __syncthreads();
    for (int r = wave; r < RGN_TH; r += 4) {
        const int li = r * RGN_TW + lane, y = y0 + r;
        if (y >= H || x >= W) continue;
        const int g = y * W + x;                               // < 2^31
        int to = g;
        if (s_key[li] >= 0) {
            const int root = s_lab[li];
            to = (y0 + root / RGN_TW) * W + tx * RGN_TW + (root % RGN_TW);
        }
        label[g] = to;
        size[g] = s_area[li];                                  // (only roots were added to)
    }
}

// ---- global union-find (launch 2): agent-scope atomics on both sides -------------------------------------------------------------------------
__device__ __forceinline__ int rgn_find_agent(int* lab, int a) {
    int p;
    while ((p = __hip_atomic_load(&lab[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != a) a = p;
    return a;
}

__device__ __forceinline__ void rgn_union_agent(int* lab, int a, int b) {
    for (;;) {
        a = rgn_find_agent(lab, a);
        b = rgn_find_agent(lab, b);
        if (a == b) return;
        if (a > b) { const int c = a; a = b; b = c; }
        const int old = atomicMin(&lab[b], a);
        if (old == b) return;
        b = old;
    }
}

// threads 0 .. nh - 1: the pixels of the rows y = RGN_TH, 2 RGN_TH ... (row k + 1 of them: idx / W); then the pixels of the columns
// x = RGN_TW, 2 RGN_TW ... (column j / H).  The id plane is read only in this launch: plain loads.
__global__ __launch_bounds__(256) void rgn_seam_kernel(const uint8_t* __restrict__ ids, int H, int W, int holes, int conn8, int* label, long nh,
                                                       long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    if (idx < nh) {
        const int k = (int)(idx / W), x = (int)(idx - (long)k * W), y = (k + 1) * RGN_TH;
        const int p = y * W + x, up = p - W;
        const int key = rgn_key(ids[p], holes);
        if (key < 0) return;
        if (ids[up] == key) rgn_union_agent(label, p, up);
        else if (conn8) {
            if (x > 0 && ids[up - 1] == key) rgn_union_agent(label, p, up - 1);
            if (x < W - 1 && ids[up + 1] == key) rgn_union_agent(label, p, up + 1);
        }
    } else {
        const long j = idx - nh;
        const int k = (int)(j / H), y = (int)(j - (long)k * H), x = (k + 1) * RGN_TW;
        const int p = y * W + x, left = p - 1;
        const int key = rgn_key(ids[p], holes);
        if (key < 0) return;
        if (ids[left] == key) rgn_union_agent(label, p, left);
        else if (conn8) {
            if (y > 0 && ids[left - W] == key) rgn_union_agent(label, p, left - W);
            if (y < H - 1 && ids[left + W] == key) rgn_union_agent(label, p, left + W);
        }
    }
}

// ---- launches 3 and 4: label[] is final behind the kernel boundary --------------------------------------------------------------------------
__device__ __forceinline__ int rgn_find(const int* lab, int a) {
    int p;
    while ((p = lab[a]) != a) a = p;
    return a;
}

__global__ __launch_bounds__(256) void rgn_size_kernel(int* label, unsigned* size, int HW) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= HW) return;
    const int p = (int)idx;
    const unsigned s = size[p];
    if (s == 0u) return;
    const int root = rgn_find(label, p);
    if (root == p) return;
    atomicAdd(&size[root], s & ~RGN_BORDER);                   // (the sum of a component's areas is at most H W < 2^31: bit 31 stays the border's)
    if (s & RGN_BORDER) atomicOr(&size[root], RGN_BORDER);
    __hip_atomic_store(&label[p], root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// counts + 0 / + 1: components rewritten / pixels rewritten (stage A: counts[0], counts[1]; stage B: counts[2], counts[3])
__global__ __launch_bounds__(256) void rgn_apply_kernel(uint8_t* ids, int HW, int holes, int limit, const int* __restrict__ label,
                                                        const unsigned* __restrict__ size, int* __restrict__ counts) {
    __shared__ int s_n[2];
    const int t = threadIdx.x;
    if (t < 2) s_n[t] = 0;
    __syncthreads();
    const long idx = (long)blockIdx.x * 256 + t;
    bool hit = false, first = false;
    if (idx < HW) {
        const int p = (int)idx;
        const int v = ids[p];
        if (holes ? v == 0 : v != 0) {
            const int root = rgn_find(label, p);
            const unsigned s = size[root];
            hit = (int)(s & ~RGN_BORDER) < limit && !(holes && (s & RGN_BORDER));
            if (hit) {
                ids[p] = holes ? ids[root - 1] : (uint8_t)0;
                first = root == p;
            }
        }
    }
    const unsigned long long hits = __ballot(hit), firsts = __ballot(first);
    if ((t & 63) == 0 && hits) {
        atomicAdd(&s_n[1], __popcll(hits));
        if (firsts) atomicAdd(&s_n[0], __popcll(firsts));
    }
    __syncthreads();
    if (t < 2 && s_n[t]) atomicAdd(&counts[t], s_n[t]);
}

__global__ void rgn_zero_kernel(int* counts) {
    if (threadIdx.x < 4) counts[threadIdx.x] = 0;
}

static void rgn_stage(uint8_t* ids, int H, int W, int holes, int conn8, int limit, int* label, unsigned* size, int* counts, bool zero, hipStream_t s) {
    const int tiles_x = (W + RGN_TW - 1) / RGN_TW, tiles_y = (H + RGN_TH - 1) / RGN_TH;
    const int HW = H * W;
    const unsigned blocks = (unsigned)(((long)HW + 255) / 256);
    hipLaunchKernelGGL(rgn_local_kernel, dim3((unsigned)tiles_x * (unsigned)tiles_y), dim3(256), 0, s, (const uint8_t*)ids, H, W, tiles_x, holes, conn8,
                       label, size, zero ? counts : (int*)nullptr);
    const long nh = (long)(tiles_y - 1) * W, total = nh + (long)(tiles_x - 1) * H;
    if (total > 0)
        hipLaunchKernelGGL(rgn_seam_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const uint8_t*)ids, H, W, holes, conn8, label, nh, total);
    hipLaunchKernelGGL(rgn_size_kernel, dim3(blocks), dim3(256), 0, s, label, size, HW);
    hipLaunchKernelGGL(rgn_apply_kernel, dim3(blocks), dim3(256), 0, s, ids, HW, holes, limit, (const int*)label, (const unsigned*)size,
                       counts + (holes ? 2 : 0));
}

// PROB_TO_ID flags == 2048.  p2 = ids u8 [i1, i2], rewritten in place; i3 = min_region, i4 = fill_holes, i5 = connectivity;
// p5 = scratch int32 [i8 + 2^31 i9]; p7 = counts int32 [4]
int launch_region_filter(const cutie_op* op, hipStream_t s) {
    const uint64_t* p = op->p;
    const int H = op->i[1], W = op->i[2], min_region = op->i[3], fill_holes = op->i[4], conn = op->i[5];
    if (H < 1 || W < 1) { cutie_set_error("region filter: empty shape (H, W >= 1)"); return -2; }
    if ((long)H * W >= (1l << 31)) { cutie_set_error("region filter: %d x %d exceeds 2^31 pixels", H, W); return -2; }
    if (min_region < 0 || fill_holes < 0) { cutie_set_error("region filter: negative threshold (min_region %d, fill_holes %d)", min_region, fill_holes); return -2; }
    if (conn != 4 && conn != 8) { cutie_set_error("region filter: connectivity %d, 4 or 8", conn); return -2; }
    if (!p[2]) { cutie_set_error("region filter: needs the id plane (p2)"); return -2; }
    if (!p[5]) { cutie_set_error("region filter: needs the scratch (p5)"); return -2; }
    if (!p[7]) { cutie_set_error("region filter: needs counts (p7)"); return -2; }
    if ((p[5] & 3) || (p[7] & 3)) { cutie_set_error("region filter: scratch and counts 4-byte aligned"); return -2; }
    const long need = 2l * H * W;
    const long words = (op->i[8] < 0 || op->i[9] < 0) ? -1l : (long)op->i[8] + ((long)op->i[9] << 31);
    if (words < need) { cutie_set_error("region filter: scratch of %ld words, %d x %d needs %ld", words, H, W, need); return -2; }
    int* label = (int*)p[5];
    unsigned* size = (unsigned*)p[5] + (long)H * W;
    int* counts = (int*)p[7];
    const bool islands = min_region >= 2, holes = fill_holes >= 2;
    if (!islands && !holes) hipLaunchKernelGGL(rgn_zero_kernel, dim3(1), dim3(64), 0, s, counts);
    if (islands) rgn_stage((uint8_t*)p[2], H, W, 0, conn == 8, min_region, label, size, counts, true, s);
    if (holes) rgn_stage((uint8_t*)p[2], H, W, 1, conn == 8, fill_holes, label, size, counts, !islands, s);
    return (int)hipGetLastError();
}
