// Baseline JPEG decode (ABI 6): the RESIZE flags 8 (Huffman), 16 (IDCT) and 32 (upsampling + colour conversion).  The packet is
// built on the host by cutie_amd/inference/data/jpeg.py (layout in its docstring, offsets in its header); the numerics are
// libjpeg's, so that the uint8 [H, W, 3] frame equals PIL's Image.open(...).convert('RGB') byte for byte.
//
// Huffman stage, per entropy-coded segment (the data between two restart markers) cut into chunks of chunk_bits bits:
//   1. speculative pass: one thread per chunk decodes from the chunk's first bit with a guessed state (block 0 of the MCU, DC next)
//      until it passes the chunk end, and records the exit (bit position, state).  The first chunk of a segment starts exact.
//   2. sync rounds: every chunk is decoded again from its predecessor's exit; a thread whose exit changed goes on into the following
//      chunks, storing their exits, until it reaches an exit equal to the stored one (the decodes have synchronised) or SYNC_AHEAD
//      chunks.  A segment whose exits did not change in a round has reached the fixed point exit[j] = decode(chunk j, exit[j-1]) with
//      exit[-1] exact, i.e. every exit is the true one; the kernels of later rounds return at once.
//   3. a segment still changing after the last round is decoded serially by one thread (counted in status[2]).  Correctness
//      never depends on the speculation.
//   4. one workgroup scans the per-chunk block counts and per-component DC difference sums (exclusive; every pass records them) and
//      checks that every segment holds its blocks.
//   5. write pass: one thread per chunk decodes from its true start, with the block index and the DC predictors the scan gives,
//      and stores the quantised coefficients (natural order, absolute DC) of the blocks it finishes or continues.
// The Huffman tables live in LDS (every workgroup copies them), so a symbol costs one LDS lookup plus, every 32 bits, a data load.
// Error bits go to status[0] (1 bad code, 2 data ends early): libjpeg substitutes zeros there with a warning, this decoder refuses the
// frame.  Everything else libjpeg accepts decodes as libjpeg decodes it: DC categories up to 15, an AC run past index 63 (stored at 63,
// ending the block, as its padded jpeg_natural_order does).  The buffers are sized from
// the packet on the host and no read or write leaves them, whatever the entropy data holds.  All stores are plain C++.
#include "common.h"

namespace {

// packet header words (cutie_amd/inference/data/jpeg.py HDR_*)
enum { H_MAGIC, H_H, H_W, H_NCOMP, H_BPM, H_MCUS_X, H_NMCU, H_RI, H_NSEG, H_NCHUNK, H_CHUNK_BITS, H_NBLOCK, H_HMAX, H_VMAX,
       H_PLANE_BYTES, H_OFF_SEG, H_OFF_C2S, H_OFF_COMP, H_OFF_MB, H_OFF_Q, H_OFF_HUFF, H_OFF_DATA, H_BYTES, H_NTAB };
enum { C_H, C_V, C_BW, C_BH, C_BLK_OFF, C_PLANE_OFF, C_PLANE_W, C_DW, C_DH, C_DC, C_AC };
constexpr int COMP_WORDS = 16, FASTBITS = 9;
constexpr int TAB_MAXCODE = 1 << FASTBITS, TAB_VALOFF = TAB_MAXCODE + 18, TAB_VAL = TAB_VALOFF + 18, TABW = TAB_VAL + 256;
constexpr int ERR_CODE = 1, ERR_TRUNC = 2;

__constant__ int kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                                13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52,
                                45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int MAX_TAB = 6, MAX_BPM = 10;

// the Huffman tables and the per-block table offsets, copied into LDS by every workgroup of the Huffman kernels: a symbol then costs one
// LDS lookup (the fast table) instead of a chain of dependent global loads
struct Lds {
    int tab[MAX_TAB * TABW];
    int dc[MAX_BPM], ac[MAX_BPM], comp[MAX_BPM];   // block b of the MCU: its DC / AC table offsets in tab, its component
};

struct Geo {                       // the packet sections the Huffman threads read
    const int* w;                  // the packet as int32 words
    const int* seg;                // [nseg][4]
    const int* comp;               // [3][COMP_WORDS]
    const int* mb;                 // [MAX_BPM][4]
    const Lds* l;
    int bpm;
};

// every thread of the workgroup calls this before any returns (it ends with a barrier)
__device__ __forceinline__ Geo load_geo(const int* w, Lds& l) {
    Geo g;
    g.w = w;
    g.seg = w + w[H_OFF_SEG];
    g.comp = w + w[H_OFF_COMP];
    g.mb = w + w[H_OFF_MB];
    g.l = &l;
    g.bpm = min(w[H_BPM], MAX_BPM);
    const int ntab = min(w[H_NTAB], MAX_TAB);
    const int* huff = w + w[H_OFF_HUFF];
    for (int i = threadIdx.x; i < ntab * TABW; i += blockDim.x) l.tab[i] = huff[i];
    if ((int)threadIdx.x < g.bpm) {
        const int b = threadIdx.x, c = min(max(g.mb[b * 4], 0), 2);
        l.comp[b] = c;
        l.dc[b] = min(max(g.comp[c * COMP_WORDS + C_DC], 0), ntab - 1) * TABW;
        l.ac[b] = min(max(g.comp[c * COMP_WORDS + C_AC], 0), ntab - 1) * TABW;
    }
    __syncthreads();
    return g;
}

// big-endian bit reader over one segment's destuffed bytes; words past the padded end read as ones (the JPEG fill bit)
struct Bits {
    const uint32_t* data;          // 4-byte aligned start of the segment
    int nwords;                    // padded length in words
    int cw = -2;                   // word index held in hi (lo holds the next one)
    uint32_t hi = 0, lo = 0;
    __device__ __forceinline__ uint32_t word(int i) const {
        return (i >= 0 && i < nwords) ? __builtin_bswap32(data[i]) : 0xffffffffu;
    }
    __device__ __forceinline__ uint32_t peek(int p) {          // the 32 bits from bit p on
        const int wi = p >> 5;
        if (wi != cw) {
            if (wi == cw + 1) { hi = lo; lo = word(wi + 1); }
            else { hi = word(wi); lo = word(wi + 1); }
            cw = wi;
        }
        const int s = p & 31;
        return s ? (hi << s) | (lo >> (32 - s)) : hi;
    }
};

// one Huffman symbol at the top of the 32-bit window -> code length (0: no such code) and symbol
__device__ __forceinline__ int huff_decode(const int* t, uint32_t win, int& sym) {
    const int e = t[win >> (32 - FASTBITS)];
    if (e) { sym = e & 255; return e >> 8; }
    for (int l = FASTBITS + 1; l <= 16; ++l) {
        const int code = (int)(win >> (32 - l));
        if (code <= t[TAB_MAXCODE + l]) {
            sym = t[TAB_VAL + min(max(code + t[TAB_VALOFF + l], 0), 255)];
            return l;
        }
    }
    sym = 0;
    return 0;
}

__device__ __forceinline__ int extend(uint32_t r, int s) { return (int)r < (1 << (s - 1)) ? (int)r - (1 << s) + 1 : (int)r; }

// decoder state: bit position p and st = b * 64 + z (block b of the MCU; z = 0 before its DC, else the zigzag index of the next
// AC coefficient); err collects error bits; dc[c] adds up component c's DC differences (from 0: the sum over a chunk; from the
// predictor: libjpeg's last_dc_val).  The decode from (p, st) is a pure function of the data: a bad code consumes 16 bits.
struct Sym {
    int p, st, err;
    int dc0, dc1, dc2;             // (three scalars, not an array indexed at run time: that would live in scratch)
    __device__ __forceinline__ int add_dc(int c, int d) {
        dc0 += c == 0 ? d : 0; dc1 += c == 1 ? d : 0; dc2 += c == 2 ? d : 0;
        return c == 0 ? dc0 : (c == 1 ? dc1 : dc2);
    }
};

// one symbol; -> true when it ends a block.  STORE: write the value into blk (the write pass; DC as the running sum)
template <bool STORE>
__device__ __forceinline__ bool step(const Geo& g, Bits& br, Sym& s, int16_t* blk) {
    const int b = s.st >> 6, z = s.st & 63;
    const uint32_t win = br.peek(s.p);
    int sym;
    if (z == 0) {
        int l = huff_decode(g.l->tab + g.l->dc[b], win, sym);
        if (!l) { l = 16; sym = 0; s.err |= ERR_CODE; }
        sym &= 15;                                              // (the parser admits no DC symbol above 15, as libjpeg)
        int diff = 0;
        if (sym) diff = extend((l + sym <= 32 ? win << l : br.peek(s.p + l)) >> (32 - sym), sym);
        s.p += l + sym;
        const int dc = s.add_dc(g.l->comp[b], diff);
        if (STORE) blk[0] = (int16_t)dc;                        // libjpeg: (JCOEF) of its int predictor
        s.st = b * 64 + 1;
        return false;
    }
    int l = huff_decode(g.l->tab + g.l->ac[b], win, sym);
    if (!l) { l = 16; sym = 0; s.err |= ERR_CODE; }
    const int r = sym >> 4, sz = sym & 15;
    int k = z;
    bool end;
    if (sz) {
        k += r;
        const uint32_t v = (l + sz <= 32 ? win << l : br.peek(s.p + l)) >> (32 - sz);
        k = min(k, 63);                                         // libjpeg: jpeg_natural_order[64..79] = 63
        if (STORE) blk[kZigzag[k]] = (int16_t)extend(v, sz);
        s.p += l + sz;
        end = k >= 63;
    } else {
        s.p += l;
        k += 15;
        end = r != 15 || k >= 63;
    }
    if (end) { s.st = b + 1 == g.bpm ? 0 : (b + 1) * 64; return true; }
    s.st = b * 64 + k + 1;
    return false;
}

__device__ __forceinline__ uint64_t pack_exit(const Sym& s) { return ((uint64_t)(uint32_t)s.st << 32) | (uint32_t)s.p; }
__device__ __forceinline__ Sym unpack_exit(uint64_t e) { return Sym{(int)(uint32_t)e, (int)(e >> 32), 0, 0, 0, 0}; }

struct Chunk {
    int seg, local, first, start_bit, bits_end;
    Bits br;
};

__device__ __forceinline__ Chunk chunk_of(const Geo& g, const uint8_t* pkt, int j, int chunk_bits) {
    Chunk c;
    c.seg = g.w[g.w[H_OFF_C2S] + j];
    const int* sg = g.seg + c.seg * 4;
    c.first = sg[2];
    c.local = j - c.first;
    const int nbits = sg[1] * 8;
    c.start_bit = c.local * chunk_bits;
    c.bits_end = c.local + 1 == sg[3] ? max(nbits, c.start_bit + 1) : min(c.start_bit + chunk_bits, nbits);
    c.br.data = (const uint32_t*)(pkt + sg[0]);
    c.br.nwords = (sg[1] + 3) / 4 + 2;
    return c;
}

// the per-chunk results of the decode passes in the work area: exits [n] (64-bit), blocks ended [n], their scan [n], DC sums
// [n][3], their scan [n][3], per-round flags [rounds + 1][nseg]
struct Work {
    uint64_t* exits;
    int *counts, *offs, *dcs, *dcoffs, *flags;
    __device__ __forceinline__ void put(int j, int ended, const Sym& s) {
        counts[j] = ended;
        dcs[3 * j] = s.dc0; dcs[3 * j + 1] = s.dc1; dcs[3 * j + 2] = s.dc2;
    }
};

// decode chunk c from s (DC sums from 0) until the position passes the chunk end; -> blocks ended
__device__ __forceinline__ int run_chunk(const Geo& g, Chunk& c, Sym& s) {
    s.dc0 = s.dc1 = s.dc2 = 0;
    int ended = 0, guard = c.bits_end - s.p + 64;              // every symbol consumes at least one bit
    while (s.p < c.bits_end && guard-- > 0) ended += step<false>(g, c.br, s, nullptr);
    return ended;
}

constexpr int HUFF_BS = 256;

// The bodies of the stages are device functions of (packet, work area, ...) so that the one-frame entry points below and the batch
// entry points further down (one image per blockIdx.y) run the same code.
__device__ __forceinline__ void spec_body(Lds& l, const uint8_t* __restrict__ pkt, Work wk, int nchunk, int chunk_bits) {
    const Geo g = load_geo((const int*)pkt, l);
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nchunk) return;
    Chunk c = chunk_of(g, pkt, j, chunk_bits);
    Sym s{c.start_bit, 0, 0, 0, 0, 0};
    wk.put(j, run_chunk(g, c, s), s);
    wk.exits[j] = pack_exit(s);
}

__global__ __launch_bounds__(HUFF_BS) void jpeg_spec_kernel(const uint8_t* __restrict__ pkt, Work wk, int nchunk, int chunk_bits) {
    __shared__ Lds l;
    spec_body(l, pkt, wk, nchunk, chunk_bits);
}

// sync round r: the chunks of segments that changed in round r - 1 (round 0: all) decode again from their predecessor's exit;
// a changed exit sets flags[r][segment] and the thread continues into the next chunks while their stored exits differ.  Exits are
// read and written as whole 64-bit words; a thread racing with a continuation may store a stale exit, which the next round sees.
constexpr int SYNC_AHEAD = 32;
__device__ __forceinline__ void sync_body(Lds& l, const uint8_t* __restrict__ pkt, Work wk, int nchunk, int nseg, int chunk_bits, int r) {
    const Geo g = load_geo((const int*)pkt, l);
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nchunk) return;
    Chunk c = chunk_of(g, pkt, j, chunk_bits);
    if (c.local == 0) return;
    if (r > 0 && !wk.flags[(r - 1) * nseg + c.seg]) return;
    Sym s = unpack_exit(__atomic_load_n(&wk.exits[j - 1], __ATOMIC_RELAXED));
    wk.put(j, run_chunk(g, c, s), s);
    uint64_t e = pack_exit(s);
    if (e == __atomic_load_n(&wk.exits[j], __ATOMIC_RELAXED)) return;
    __atomic_store_n(&wk.exits[j], e, __ATOMIC_RELAXED);
    wk.flags[r * nseg + c.seg] = 1;
    const int last = c.first + g.seg[c.seg * 4 + 3] - 1;
    for (int k = j + 1; k <= min(last, j + SYNC_AHEAD); ++k) {
        Chunk n = chunk_of(g, pkt, k, chunk_bits);
        const int ended = run_chunk(g, n, s);
        e = pack_exit(s);
        if (e == __atomic_load_n(&wk.exits[k], __ATOMIC_RELAXED)) break;
        __atomic_store_n(&wk.exits[k], e, __ATOMIC_RELAXED);
        wk.put(k, ended, s);
    }
}

__global__ __launch_bounds__(HUFF_BS) void jpeg_sync_kernel(const uint8_t* __restrict__ pkt, Work wk, int nchunk, int nseg, int chunk_bits,
                                                            int r) {
    __shared__ Lds l;
    sync_body(l, pkt, wk, nchunk, nseg, chunk_bits, r);
}

// status[1] = max over segments of the rounds until no change (rounds + 1: serial); a segment that still changed in the last round
// is decoded by one thread from its start (status[2] counts them)
__device__ __forceinline__ void serial_body(Lds& l, const uint8_t* __restrict__ pkt, Work wk, int* __restrict__ status, int nseg,
                                            int chunk_bits, int rounds) {
    const Geo g = load_geo((const int*)pkt, l);
    const int si = blockIdx.x * blockDim.x + threadIdx.x;
    if (si >= nseg) return;
    int used = rounds + 1;
    for (int r = 0; r < rounds; ++r)
        if (!wk.flags[r * nseg + si]) { used = r + 1; break; }
    atomicMax(status + 1, used);
    if (used <= rounds) return;
    atomicAdd(status + 2, 1);
    const int first = g.seg[si * 4 + 2], nch = g.seg[si * 4 + 3];
    Sym s{0, 0, 0, 0, 0, 0};
    for (int j = first; j < first + nch; ++j) {
        Chunk c = chunk_of(g, pkt, j, chunk_bits);
        wk.put(j, run_chunk(g, c, s), s);
        wk.exits[j] = pack_exit(s);
    }
}

__global__ __launch_bounds__(64) void jpeg_serial_kernel(const uint8_t* __restrict__ pkt, Work wk, int* __restrict__ status, int nseg,
                                                         int chunk_bits, int rounds) {
    __shared__ Lds l;
    serial_body(l, pkt, wk, status, nseg, chunk_bits, rounds);
}

constexpr int SCAN_BS = 1024;

// inclusive workgroup scan of v over SCAN_BS threads
__device__ __forceinline__ int block_scan(int* part, int v) {
    const int t = threadIdx.x;
    __syncthreads();
    part[t] = v;
    __syncthreads();
    for (int d = 1; d < SCAN_BS; d <<= 1) {
        const int u = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += u;
        __syncthreads();
    }
    return part[t];
}

// one workgroup: offs / dcoffs = exclusive scans of the chunk block counts / DC sums (over all chunks; a segment subtracts the value
// at its first chunk); every segment must end at least the blocks of its MCUs
__device__ __forceinline__ void scan_body(int* part, const uint8_t* __restrict__ pkt, Work wk, int* __restrict__ status, int nchunk) {
    const int* w = (const int*)pkt;
    const int t = threadIdx.x, per = (nchunk + SCAN_BS - 1) / SCAN_BS;
    const int lo = min(t * per, nchunk), hi = min(lo + per, nchunk);
    for (int a = 0; a < 4; ++a) {                              // block counts, then the DC sums of the three components
        const int* in = a ? wk.dcs + (a - 1) : wk.counts;
        int* out = a ? wk.dcoffs + (a - 1) : wk.offs;
        const int st = a ? 3 : 1;
        int sum = 0;
        for (int j = lo; j < hi; ++j) sum += in[j * st];
        int run = block_scan(part, sum) - sum;
        for (int j = lo; j < hi; ++j) { out[j * st] = run; run += in[j * st]; }
    }
    __syncthreads();
    const int nseg = w[H_NSEG], ri = w[H_RI], nmcu = w[H_NMCU], bpm = w[H_BPM];
    const int* seg = w + w[H_OFF_SEG];
    for (int si = t; si < nseg; si += SCAN_BS) {
        const int first = seg[si * 4 + 2], last = first + seg[si * 4 + 3] - 1;
        if (wk.offs[last] + wk.counts[last] - wk.offs[first] < (min((si + 1) * ri, nmcu) - si * ri) * bpm) atomicOr(status, ERR_TRUNC);
    }
}

__global__ __launch_bounds__(SCAN_BS) void jpeg_scan_kernel(const uint8_t* __restrict__ pkt, Work wk, int* __restrict__ status, int nchunk) {
    __shared__ int part[SCAN_BS];
    scan_body(part, pkt, wk, status, nchunk);
}

// block ordinal in scan order -> coefficient block index
__device__ __forceinline__ int block_index(const Geo& g, int mcus_x, int ordinal) {
    const int m = ordinal / g.bpm, b = ordinal - m * g.bpm;
    const int my = m / mcus_x, mx = m - my * mcus_x;
    const int* mb = g.mb + b * 4;
    const int* cw = g.comp + g.l->comp[b] * COMP_WORDS;
    return cw[C_BLK_OFF] + (my * cw[C_V] + mb[2]) * cw[C_BW] + mx * cw[C_H] + mb[1];
}

__device__ __forceinline__ void write_body(Lds& l, const uint8_t* __restrict__ pkt, Work wk, int16_t* __restrict__ coef,
                                           int* __restrict__ status, int nchunk, int chunk_bits, int nblock) {
    const Geo g = load_geo((const int*)pkt, l);
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nchunk) return;
    Chunk c = chunk_of(g, pkt, j, chunk_bits);
    const int ri = g.w[H_RI], nmcu = g.w[H_NMCU], mcus_x = g.w[H_MCUS_X];
    const int m0 = c.seg * ri, need = (min(m0 + ri, nmcu) - m0) * g.bpm, nbits = g.seg[c.seg * 4 + 1] * 8;
    int n = wk.offs[j] - wk.offs[c.first];                     // blocks of the segment ended before this chunk
    Sym s = c.local ? unpack_exit(wk.exits[j - 1]) : Sym{0, 0, 0, 0, 0, 0};
    s.dc0 = wk.dcoffs[3 * j] - wk.dcoffs[3 * c.first];       // the DC predictors
    s.dc1 = wk.dcoffs[3 * j + 1] - wk.dcoffs[3 * c.first + 1];
    s.dc2 = wk.dcoffs[3 * j + 2] - wk.dcoffs[3 * c.first + 2];
    int guard = c.bits_end - s.p + 64;
    while (s.p < c.bits_end && n < need && guard-- > 0) {
        const int bi = block_index(g, mcus_x, m0 * g.bpm + n);
        n += step<true>(g, c.br, s, coef + (long)min(max(bi, 0), nblock - 1) * 64);
        if (s.p > nbits) s.err |= ERR_TRUNC;
    }
    if (s.err) atomicOr(status, s.err);
}

__global__ __launch_bounds__(HUFF_BS) void jpeg_write_kernel(const uint8_t* __restrict__ pkt, Work wk, int16_t* __restrict__ coef,
                                                             int* __restrict__ status, int nchunk, int chunk_bits, int nblock) {
    __shared__ Lds l;
    write_body(l, pkt, wk, coef, status, nchunk, chunk_bits, nblock);
}

// ---- IDCT: libjpeg's jpeg_idct_islow (jidctint.c) in its JLONG (64-bit) arithmetic; 8 threads per block ---------------------------
constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr long FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270,
               FIX_0_899976223 = 7373, FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137,
               FIX_1_961570560 = 16069, FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

__device__ __forceinline__ void idct_1d(const long x[8], long o[8]) {      // the 8 outputs before descaling
    long z1 = (x[2] + x[6]) * FIX_0_541196100;
    const long tmp2 = z1 + x[6] * -FIX_1_847759065, tmp3 = z1 + x[2] * FIX_0_765366865;
    const long tmp0 = (x[0] + x[4]) * (1L << CONST_BITS), tmp1 = (x[0] - x[4]) * (1L << CONST_BITS);
    const long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    long t0 = x[7], t1 = x[5], t2 = x[3], t3 = x[1];
    z1 = t0 + t3;
    long z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const long z5 = (z3 + z4) * FIX_1_175875602;
    t0 *= FIX_0_298631336; t1 *= FIX_2_053119869; t2 *= FIX_3_072711026; t3 *= FIX_1_501321110;
    z1 *= -FIX_0_899976223; z2 *= -FIX_2_562915447;
    z3 = z3 * -FIX_1_961570560 + z5; z4 = z4 * -FIX_0_390180644 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    o[0] = tmp10 + t3; o[7] = tmp10 - t3; o[1] = tmp11 + t2; o[6] = tmp11 - t2;
    o[2] = tmp12 + t1; o[5] = tmp12 - t1; o[3] = tmp13 + t0; o[4] = tmp13 - t0;
}

__device__ __forceinline__ uint32_t range_limit(int x) {         // sample_range_limit + CENTERJSAMPLE at x & 1023 (jdmaster.c)
    const int u = (x + 128) & 1023;
    return u < 256 ? (uint32_t)u : (u < 640 ? 255u : 0u);
}

constexpr int IDCT_BS = 256;
__device__ __forceinline__ void idct_body(int (*ws)[65], const uint8_t* __restrict__ pkt, const int16_t* __restrict__ coef,
                                          uint8_t* __restrict__ planes, int nblock, long plane_bytes) {
    const int* w = (const int*)pkt;
    const int lb = threadIdx.x >> 3, t = threadIdx.x & 7;
    const int g = blockIdx.x * (IDCT_BS / 8) + lb;
    const bool live = g < nblock;
    const int* comp = w + w[H_OFF_COMP];
    int c = 0;
    for (int k = 1; k < w[H_NCOMP]; ++k)
        if (g >= comp[k * COMP_WORDS + C_BLK_OFF]) c = k;
    const int* cw = comp + c * COMP_WORDS;
    if (live) {                                                // pass 1: column t, dequantised in int
        const int16_t* in = coef + (long)g * 64;
        const int* q = w + w[H_OFF_Q] + c * 64;
        long x[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = (long)in[k * 8 + t] * q[k * 8 + t];
        idct_1d(x, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) ws[lb][k * 8 + t] = (int)((o[k] + (1L << (CONST_BITS - PASS1_BITS - 1))) >> (CONST_BITS - PASS1_BITS));
    }
    __syncthreads();
    if (!live) return;
    long x[8], o[8];                                           // pass 2: row t
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = ws[lb][t * 8 + k];
    idct_1d(x, o);
    constexpr int SH = CONST_BITS + PASS1_BITS + 3;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lo |= range_limit((int)((o[k] + (1L << (SH - 1))) >> SH)) << (8 * k);
        hi |= range_limit((int)((o[k + 4] + (1L << (SH - 1))) >> SH)) << (8 * k);
    }
    const int rel = g - cw[C_BLK_OFF], bw = cw[C_BW];
    const int by = rel / bw, bx = rel - by * bw;
    const long off = (long)cw[C_PLANE_OFF] + (long)(by * 8 + t) * cw[C_PLANE_W] + bx * 8;
    if (off >= 0 && off + 8 <= plane_bytes) {
        uint32_t* out = (uint32_t*)(planes + off);             // 8-byte aligned: plane offsets and widths are multiples of 8
        out[0] = lo;
        out[1] = hi;
    }
}

__global__ __launch_bounds__(IDCT_BS) void jpeg_idct_kernel(const uint8_t* __restrict__ pkt, const int16_t* __restrict__ coef,
                                                            uint8_t* __restrict__ planes, int nblock, long plane_bytes) {
    __shared__ int ws[IDCT_BS / 8][65];
    idct_body(ws, pkt, coef, planes, nblock, plane_bytes);
}

// ---- upsampling (jdsample.c) + YCbCr -> RGB (jdcolor.c, SCALEBITS 16) ------------------------------------------------------------
__device__ __forceinline__ int px(const uint8_t* p, int pw, int y, int x) { return p[(long)y * pw + x]; }

// chroma sample of output pixel (x, y): plane p (pw wide), downsampled extent dw x dh.  Fancy h1v2 always, fancy h2v1 / h2v2 where
// dw > 2, else replication; the neighbour row past the extent repeats its edge row
__device__ __forceinline__ int chroma(const uint8_t* p, int pw, int dw, int dh, int hmax, int vmax, int x, int y) {
    if (hmax == 1 && vmax == 1) return px(p, pw, y, x);
    const int i = hmax == 2 ? x >> 1 : x, j = vmax == 2 ? y >> 1 : y;
    if (hmax == 2 && dw <= 2) return px(p, pw, j, i);
    if (vmax == 1) {                                           // h2v1
        const int c0 = px(p, pw, j, i);
        if (x & 1) return i == dw - 1 ? c0 : (3 * c0 + px(p, pw, j, i + 1) + 2) >> 2;
        return i == 0 ? c0 : (3 * c0 + px(p, pw, j, i - 1) + 1) >> 2;
    }
    const int nb = (y & 1) ? min(j + 1, dh - 1) : max(j - 1, 0);
    if (hmax == 1) return (3 * px(p, pw, j, i) + px(p, pw, nb, i) + ((y & 1) ? 2 : 1)) >> 2;      // h1v2
    const int cs = 3 * px(p, pw, j, i) + px(p, pw, nb, i);                                        // h2v2: column sums
    if (x & 1) return i == dw - 1 ? (cs * 4 + 7) >> 4 : (3 * cs + 3 * px(p, pw, j, i + 1) + px(p, pw, nb, i + 1) + 7) >> 4;
    return i == 0 ? (cs * 4 + 8) >> 4 : (3 * cs + 3 * px(p, pw, j, i - 1) + px(p, pw, nb, i - 1) + 8) >> 4;
}

__device__ __forceinline__ uint8_t clamp255(int v) { return (uint8_t)min(max(v, 0), 255); }

__device__ __forceinline__ void color_body(const uint8_t* __restrict__ pkt, const uint8_t* __restrict__ planes, uint8_t* __restrict__ rgb,
                                           int H, int W, long ld) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)H * W) return;
    const int y = (int)(idx / W), x = (int)(idx - (long)y * W);
    const int* w = (const int*)pkt;
    const int* comp = w + w[H_OFF_COMP];
    const int Y = px(planes + comp[C_PLANE_OFF], comp[C_PLANE_W], y, x);
    uint8_t* o = rgb + (long)y * ld + (long)x * 3;
    if (w[H_NCOMP] == 1) { o[0] = o[1] = o[2] = (uint8_t)Y; return; }
    const int hmax = w[H_HMAX], vmax = w[H_VMAX];
    const int* c1 = comp + COMP_WORDS;
    const int* c2 = comp + 2 * COMP_WORDS;
    const int cb = chroma(planes + c1[C_PLANE_OFF], c1[C_PLANE_W], c1[C_DW], c1[C_DH], hmax, vmax, x, y) - 128;
    const int cr = chroma(planes + c2[C_PLANE_OFF], c2[C_PLANE_W], c2[C_DW], c2[C_DH], hmax, vmax, x, y) - 128;
    o[0] = clamp255(Y + ((91881 * cr + 32768) >> 16));
    o[1] = clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    o[2] = clamp255(Y + ((116130 * cb + 32768) >> 16));
}

__global__ void jpeg_color_kernel(const uint8_t* __restrict__ pkt, const uint8_t* __restrict__ planes, uint8_t* __restrict__ rgb,
                                  int H, int W, long ld) {
    color_body(pkt, planes, rgb, H, W, ld);
}

// ---- batch forms (flags & 256; include/cutie_hip.h, ABI 11, forms added): N images through one chain of launches ---------------------
// The image index is blockIdx.y (blockIdx.x for the scan, one workgroup per image); the grids are sized for the largest image of the
// batch and the workgroups past an image's own count return.  Table and packet headers are device data: every entry point checks the
// image's row and header against the totals of the descriptor (load_img) before it touches anything else of the image, and skips an
// image that fails (error bit 4).  The check is a pure function of data that no stage writes, so every stage decides alike.
constexpr int ERR_TABLE = 4, MAGIC = 0x3147504A, HDR_WORDS = 64;
enum { R_PKT, R_WORK, R_COEF, R_PLANES, R_RGB, R_PKT_BYTES, R_LD, R_RESERVED, ROW_WORDS };

struct Batch {                     // the descriptor: buffer bases, their extents, the grid bounds
    const uint8_t* pkts;
    const int* tab;
    int* work;
    int16_t* coef;
    uint8_t *planes, *rgb;
    int* status;
    long pkt_bytes, work_words, coef_elems, plane_bytes, rgb_bytes, max_pix;
    int n, rounds, max_chunk, max_seg, max_block;
};

struct Img {                       // one image of the batch: what the one-frame launcher passes to the kernels
    const uint8_t* pkt;
    Work wk;
    int16_t* coef;
    uint8_t *planes, *rgb;
    int* status;
    long plane_bytes, ld;
    int nchunk, nseg, nblock, chunk_bits, H, W;
};

__device__ __forceinline__ bool section(long off, long n, long words) { return off >= HDR_WORDS && off + n <= words; }

// row k and its packet header against the descriptor -> the image's pointers; false: bad table or header, nothing of the image is used
__device__ __forceinline__ bool load_img(const Batch& b, int k, Img& m) {
    const int* r = b.tab + (long)k * ROW_WORDS;
    m.status = b.status + 4L * k;
    const long po = r[R_PKT], pb = r[R_PKT_BYTES];
    if (po < 0 || (po & 15) || pb < 4 * HDR_WORDS || (pb & 3) || po + pb > b.pkt_bytes) return false;
    const int* h = (const int*)(b.pkts + po);
    if (h[H_MAGIC] != MAGIC || h[H_BYTES] != pb) return false;
    const long words = pb >> 2, nchunk = h[H_NCHUNK], nseg = h[H_NSEG], nblock = h[H_NBLOCK], ncomp = h[H_NCOMP], H = h[H_H], W = h[H_W];
    if (nchunk < 1 || nchunk > b.max_chunk || nseg < 1 || nseg > b.max_seg || nblock < 1 || nblock > b.max_block) return false;
    if (H < 1 || W < 1 || H * W > b.max_pix || (ncomp != 1 && ncomp != 3) || h[H_CHUNK_BITS] < 64) return false;
    if (h[H_BPM] < 1 || h[H_BPM] > MAX_BPM || h[H_NTAB] < 1 || h[H_NTAB] > MAX_TAB || h[H_MCUS_X] < 1 || h[H_NMCU] < 1 || h[H_RI] < 1 ||
        h[H_HMAX] < 1 || h[H_HMAX] > 2 || h[H_VMAX] < 1 || h[H_VMAX] > 2)
        return false;
    if (!section(h[H_OFF_SEG], 4 * nseg, words) || !section(h[H_OFF_C2S], nchunk, words) || !section(h[H_OFF_COMP], 3 * COMP_WORDS, words) ||
        !section(h[H_OFF_MB], 4 * MAX_BPM, words) || !section(h[H_OFF_Q], 64 * ncomp, words) ||
        !section(h[H_OFF_HUFF], (long)h[H_NTAB] * TABW, words) || h[H_OFF_DATA] < 4 * HDR_WORDS || h[H_OFF_DATA] > pb)
        return false;
    // the work area ends where the next image's begins: the chunks and segments of the header must fit what the host laid out
    const long wo = r[R_WORK], wend = k + 1 < b.n ? (long)b.tab[(long)(k + 1) * ROW_WORDS + R_WORK] : b.work_words;
    if (wo < 0 || (wo & 1) || wend < wo || wend > b.work_words || 10 * nchunk + (b.rounds + 1) * nseg > wend - wo) return false;
    const long co = r[R_COEF], plo = r[R_PLANES], ro = r[R_RGB], ld = r[R_LD], plane_bytes = h[H_PLANE_BYTES];
    if (co < 0 || (co & 7) || co + 64 * nblock > b.coef_elems) return false;
    if (plo < 0 || (plo & 7) || plane_bytes < 64 * nblock || plo + plane_bytes > b.plane_bytes) return false;
    if (ro < 0 || (ro & 15) || ld < 3 * W || ro + (H - 1) * ld + 3 * W > b.rgb_bytes) return false;
    m.pkt = b.pkts + po;
    int* wk = b.work + wo;
    m.wk.exits = (uint64_t*)wk;
    m.wk.counts = wk + 2 * nchunk;
    m.wk.offs = m.wk.counts + nchunk;
    m.wk.dcs = m.wk.offs + nchunk;
    m.wk.dcoffs = m.wk.dcs + 3 * nchunk;
    m.wk.flags = m.wk.dcoffs + 3 * nchunk;
    m.coef = b.coef + co;
    m.planes = b.planes + plo;
    m.rgb = b.rgb + ro;
    m.plane_bytes = plane_bytes;
    m.ld = ld;
    m.nchunk = (int)nchunk; m.nseg = (int)nseg; m.nblock = (int)nblock; m.chunk_bits = h[H_CHUNK_BITS]; m.H = (int)H; m.W = (int)W;
    return true;
}

// the whole workgroup takes the same branch (the image is per workgroup), so a return here is in front of every barrier
#define JPEG_BATCH_IMAGE(b, k, m, live)                                                   \
    Img m;                                                                                \
    if (!load_img(b, k, m)) {                                                             \
        if (threadIdx.x == 0 && (live)) atomicOr(m.status, ERR_TABLE);                    \
        return;                                                                           \
    }

// per-round flags and coefficients of every image to 0.  A kernel and not memsets: the images' regions are apart (other rows' data,
// guard bytes of the tests lie between them), so memsets would be one per image and buffer; this is one launch whatever N is.
__global__ __launch_bounds__(256) void jpeg_clear_batch_kernel(Batch b) {
    JPEG_BATCH_IMAGE(b, blockIdx.y, m, blockIdx.x == 0)
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < (long)(b.rounds + 1) * m.nseg) m.wk.flags[t] = 0;
    if (t < 8L * m.nblock) ((uint4*)m.coef)[t] = uint4{0, 0, 0, 0};         // (16-byte aligned: base and offset are)
}

__global__ __launch_bounds__(HUFF_BS) void jpeg_spec_batch_kernel(Batch b) {
    __shared__ Lds l;
    JPEG_BATCH_IMAGE(b, blockIdx.y, m, false)
    if ((int)(blockIdx.x * HUFF_BS) >= m.nchunk) return;                      // (before the table copy: a small image beside a large one)
    spec_body(l, m.pkt, m.wk, m.nchunk, m.chunk_bits);
}

__global__ __launch_bounds__(HUFF_BS) void jpeg_sync_batch_kernel(Batch b, int r) {
    __shared__ Lds l;
    JPEG_BATCH_IMAGE(b, blockIdx.y, m, false)
    if ((int)(blockIdx.x * HUFF_BS) >= m.nchunk) return;
    sync_body(l, m.pkt, m.wk, m.nchunk, m.nseg, m.chunk_bits, r);
}

__global__ __launch_bounds__(64) void jpeg_serial_batch_kernel(Batch b) {
    __shared__ Lds l;
    JPEG_BATCH_IMAGE(b, blockIdx.y, m, false)
    if ((int)(blockIdx.x * 64) >= m.nseg) return;
    serial_body(l, m.pkt, m.wk, m.status, m.nseg, m.chunk_bits, b.rounds);
}

__global__ __launch_bounds__(SCAN_BS) void jpeg_scan_batch_kernel(Batch b) {
    __shared__ int part[SCAN_BS];
    JPEG_BATCH_IMAGE(b, blockIdx.x, m, false)
    scan_body(part, m.pkt, m.wk, m.status, m.nchunk);
}

__global__ __launch_bounds__(HUFF_BS) void jpeg_write_batch_kernel(Batch b) {
    __shared__ Lds l;
    JPEG_BATCH_IMAGE(b, blockIdx.y, m, false)
    if ((int)(blockIdx.x * HUFF_BS) >= m.nchunk) return;
    write_body(l, m.pkt, m.wk, m.coef, m.status, m.nchunk, m.chunk_bits, m.nblock);
}

// (the IDCT and colour stages may be launched on their own, so they set the error bit too)
__global__ __launch_bounds__(IDCT_BS) void jpeg_idct_batch_kernel(Batch b) {
    __shared__ int ws[IDCT_BS / 8][65];
    JPEG_BATCH_IMAGE(b, blockIdx.y, m, blockIdx.x == 0)
    if ((int)(blockIdx.x * (IDCT_BS / 8)) >= m.nblock) return;
    idct_body(ws, m.pkt, m.coef, m.planes, m.nblock, m.plane_bytes);
}

__global__ __launch_bounds__(256) void jpeg_color_batch_kernel(Batch b) {
    JPEG_BATCH_IMAGE(b, blockIdx.y, m, blockIdx.x == 0)
    color_body(m.pkt, m.planes, m.rgb, m.H, m.W, m.ld);
}

}  // namespace

#define GRID1D(n, bs) dim3((unsigned)(((long)(n) + (bs) - 1) / (bs)))

// RESIZE flags 8 / 16 / 32 with flags & 256 (include/cutie_hip.h, ABI 11, forms added): the stages over i0 images, one launch each
static int launch_jpeg_batch(const cutie_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    const uint64_t* p = op->p;
    if (op->flags & ~(256 | 56)) { cutie_set_error("jpeg batch: flags 8 / 16 / 32 with 256, nothing else"); return -2; }
    Batch b;
    b.pkts = (const uint8_t*)p[0]; b.tab = (const int*)p[1]; b.work = (int*)p[2]; b.coef = (int16_t*)p[3];
    b.planes = (uint8_t*)p[4]; b.rgb = (uint8_t*)p[5]; b.status = (int*)p[6];
    b.n = i[0]; b.pkt_bytes = i[1]; b.work_words = i[2]; b.coef_elems = i[3]; b.plane_bytes = i[4]; b.rgb_bytes = i[5];
    b.rounds = i[6]; b.max_chunk = i[7]; b.max_seg = i[8]; b.max_block = i[9]; b.max_pix = i[10];
    if (b.n < 1 || b.n > 65535) { cutie_set_error("jpeg batch: %d images (1 .. 65535)", b.n); return -2; }
    if (!p[0] || !p[1] || !p[6] || ((p[0] | p[1] | p[6]) & 15) || b.pkt_bytes < 256) {
        cutie_set_error("jpeg batch: packets (p0, i1 bytes), table (p1) and status (p6), 16-byte aligned");
        return -2;
    }
    if (b.rounds < 0 || b.rounds > 64 || b.max_chunk < 1 || b.max_seg < 1 || b.max_block < 1 || b.max_pix < 1) {
        cutie_set_error("jpeg batch: bad bounds (rounds %d, chunks %d, segments %d, blocks %d, pixels %ld)", b.rounds, b.max_chunk, b.max_seg,
                        b.max_block, b.max_pix);
        return -2;
    }
    const unsigned N = (unsigned)b.n;
    if (op->flags & 8) {
        if (!p[2] || !p[3] || (p[2] & 7) || (p[3] & 15) || b.work_words < 1 || b.coef_elems < 64) {
            cutie_set_error("jpeg batch: the Huffman stage needs work (p2, 8-byte aligned, i2 words) and coef (p3, 16-byte aligned, i3 elements)");
            return -2;
        }
        const long clear = std::max(8L * b.max_block, (long)(b.rounds + 1) * b.max_seg);
        const dim3 huff(GRID1D(b.max_chunk, HUFF_BS).x, N);
        hipMemsetAsync(b.status, 0, sizeof(int) * 4 * (size_t)b.n, s);
        hipLaunchKernelGGL(jpeg_clear_batch_kernel, dim3(GRID1D(clear, 256).x, N), dim3(256), 0, s, b);
        hipLaunchKernelGGL(jpeg_spec_batch_kernel, huff, dim3(HUFF_BS), 0, s, b);
        for (int r = 0; r < b.rounds; ++r) hipLaunchKernelGGL(jpeg_sync_batch_kernel, huff, dim3(HUFF_BS), 0, s, b, r);
        hipLaunchKernelGGL(jpeg_serial_batch_kernel, dim3(GRID1D(b.max_seg, 64).x, N), dim3(64), 0, s, b);
        hipLaunchKernelGGL(jpeg_scan_batch_kernel, dim3(N), dim3(SCAN_BS), 0, s, b);
        hipLaunchKernelGGL(jpeg_write_batch_kernel, huff, dim3(HUFF_BS), 0, s, b);
    }
    if (op->flags & 16) {
        if (!p[3] || !p[4] || (p[3] & 15) || (p[4] & 7) || b.plane_bytes < 64) {
            cutie_set_error("jpeg batch: the IDCT stage needs coef (p3, 16-byte aligned) and planes (p4, 8-byte aligned, i4 bytes)");
            return -2;
        }
        hipLaunchKernelGGL(jpeg_idct_batch_kernel, dim3(GRID1D(b.max_block, IDCT_BS / 8).x, N), dim3(IDCT_BS), 0, s, b);
    }
    if (op->flags & 32) {
        if (!p[4] || !p[5] || (p[4] & 7) || (p[5] & 15) || b.rgb_bytes < 3) {
            cutie_set_error("jpeg batch: the colour stage needs planes (p4, 8-byte aligned) and rgb (p5, 16-byte aligned, i5 bytes)");
            return -2;
        }
        hipLaunchKernelGGL(jpeg_color_batch_kernel, dim3(GRID1D(b.max_pix, 256).x, N), dim3(256), 0, s, b);
    }
    return (int)hipGetLastError();
}

// RESIZE flags 8 / 16 / 32 (include/cutie_hip.h, ABI 6): the stages whose flag is set, in order
int launch_jpeg(const cutie_op* op, hipStream_t s) {
    if (op->flags & 256) return launch_jpeg_batch(op, s);
    const int32_t* i = op->i;
    const uint64_t* p = op->p;
    const int nchunk = i[0], nseg = i[1], nblock = i[2], chunk_bits = i[3], rounds = i[4], H = i[7], W = i[8], ncomp = i[10];
    const long plane_bytes = i[6], work_words = i[9];
    const int BS = 256;
    if (op->flags & 7) { cutie_set_error("jpeg: flags 8 / 16 / 32 cannot be combined with flags 1 / 2 / 4"); return -2; }
    if (!p[0] || i[5] < 256 || ((uintptr_t)p[0] & 3)) { cutie_set_error("jpeg: no packet (p0, 4-byte aligned, i5 bytes)"); return -2; }
    const uint8_t* pkt = (const uint8_t*)p[0];
    if (op->flags & 8) {
        if (nchunk < 1 || nseg < 1 || nblock < 1 || chunk_bits < 64 || rounds < 0 || rounds > 64 || (ncomp != 1 && ncomp != 3)) {
            cutie_set_error("jpeg: bad Huffman geometry (chunks %d, segments %d, blocks %d, chunk bits %d, rounds %d, components %d)",
                            nchunk, nseg, nblock, chunk_bits, rounds, ncomp);
            return -2;
        }
        if (!p[1] || !p[2] || !p[3] || work_words < 10L * nchunk + (long)(rounds + 1) * nseg || ((uintptr_t)p[1] & 7)) {
            cutie_set_error("jpeg: the Huffman stage needs work (8-byte aligned, 10 * chunks + (rounds + 1) * segments words), coef, status");
            return -2;
        }
        Work wk;
        wk.exits = (uint64_t*)p[1];
        wk.counts = (int*)p[1] + 2L * nchunk;
        wk.offs = wk.counts + nchunk;
        wk.dcs = wk.offs + nchunk;
        wk.dcoffs = wk.dcs + 3L * nchunk;
        wk.flags = wk.dcoffs + 3L * nchunk;
        int* status = (int*)p[3];
        int16_t* coef = (int16_t*)p[2];
        hipMemsetAsync(wk.flags, 0, sizeof(int) * (size_t)(rounds + 1) * nseg, s);
        hipMemsetAsync(status, 0, sizeof(int) * 4, s);
        hipMemsetAsync(coef, 0, sizeof(int16_t) * 64 * (size_t)nblock, s);
        hipLaunchKernelGGL(jpeg_spec_kernel, GRID1D(nchunk, HUFF_BS), dim3(HUFF_BS), 0, s, pkt, wk, nchunk, chunk_bits);
        for (int r = 0; r < rounds; ++r)
            hipLaunchKernelGGL(jpeg_sync_kernel, GRID1D(nchunk, HUFF_BS), dim3(HUFF_BS), 0, s, pkt, wk, nchunk, nseg, chunk_bits, r);
        hipLaunchKernelGGL(jpeg_serial_kernel, GRID1D(nseg, 64), dim3(64), 0, s, pkt, wk, status, nseg, chunk_bits, rounds);
        hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(SCAN_BS), 0, s, pkt, wk, status, nchunk);
        hipLaunchKernelGGL(jpeg_write_kernel, GRID1D(nchunk, HUFF_BS), dim3(HUFF_BS), 0, s, pkt, wk, coef, status, nchunk, chunk_bits, nblock);
    }
    if (op->flags & 16) {
        if (!p[2] || !p[4] || nblock < 1 || plane_bytes < 64L * nblock || ((uintptr_t)p[4] & 7)) {
            cutie_set_error("jpeg: the IDCT stage needs coef and planes (8-byte aligned, >= 64 * blocks bytes)");
            return -2;
        }
        hipLaunchKernelGGL(jpeg_idct_kernel, GRID1D(nblock, IDCT_BS / 8), dim3(IDCT_BS), 0, s, pkt, (const int16_t*)p[2], (uint8_t*)p[4],
                           nblock, plane_bytes);
    }
    if (op->flags & 32) {
        if (!p[4] || !p[5] || H < 1 || W < 1 || i[11] < 3 * W) { cutie_set_error("jpeg: the colour stage needs planes, rgb and a row stride >= 3 W"); return -2; }
        hipLaunchKernelGGL(jpeg_color_kernel, GRID1D((long)H * W, BS), dim3(BS), 0, s, pkt, (const uint8_t*)p[4], (uint8_t*)p[5], H, W,
                           (long)i[11]);
    }
    return (int)hipGetLastError();
}
