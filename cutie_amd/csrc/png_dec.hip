// RESIZE flags 64 / 128 (ABI 11, forms added): mask PNGs decoded on the device -- inflate (RFC 1950 / 1951) and PNG unfilter + unpack -- for the scorer
// (SequenceScorer gt_decode='device', score_masks --decode device; packets: cutie_amd/inference/data/png_packet.py; the Python model:
// tests/png_dec_ref.py).  The result equals np.array(Image.open(f)) byte for byte.
//
// One launch takes N images, one wave64 (= one block) per image: a DEFLATE stream is serial, the throughput comes from the batch.
//
//   png_inflate_kernel   lane 0 runs the serial core (png_inflate_core.h: bit reader, code tables in LDS, symbol decode and EVERY bounds check)
//                        and fills an LDS queue of up to 64 tokens; then the whole wave executes the queue: the literals are scattered,
//                        one per lane; every match is copied by all lanes, out[pos + i] = out[pos - dist + (i % dist)], which is right for
//                        overlapping matches (distance-1 runs) too, because it reads only bytes in front of the match; a stored run is a
//                        copy from the packet.  The window is the output itself, in global memory.  A match that reads bytes written
//                        since the last barrier waits for a barrier first (a block is one wave on one CU: __syncthreads makes its
//                        stores visible to its loads).  At the end the wave sums the Adler-32 of the output (the composition of png.hip:
//                        A = 1 + sum b_i, B = n + sum (n - i) b_i, all mod 65521) and lane 0 compares it with the trailer.
//   png_unfilter_kernel  rows in order, the current and the previous row in LDS: filters 0 (None) and 2 (Up) lane-parallel, 1 (Sub) as a wave
//                        prefix sum mod 256 per channel (shuffle offsets bpp, 2 bpp, ...; bpp = 3 for RGB, else 1 -- on the packed bytes for
//                        depths below 8), 3 (Average) and 4 (Paeth) by one serial lane; then the row is written, pixels of 1 / 2 / 4 bits
//                        unpacked MSB first.
//
// Bad input ends in an error bit of the image's status block and in nothing else:
//   - the packet header and the table entry are device data, so both kernels check them again (pd_header; offsets inside the three buffers
//     whose sizes the launcher passes) before anything else is read; an image that fails gets PD_E_HEADER and is left alone;
//   - every read of the stream, every write of the output and every match source is checked by the core at decode time (its header has the
//     argument); the wave only executes tokens that passed;
//   - every turn of the decode loop hands out at least one token (>= 1 output byte) or consumed at least one bit or ends the loop, so the
//     work is bounded by 8 * stream bytes + inflated bytes; the unfilter stage is H rows of rowbytes steps;
//   - an image with an error bit is not unfiltered; the other images of the launch are not affected (nothing is shared between blocks).
#include "common.h"
#include "png_inflate_core.h"

#define PNGD_QUEUE 64
#define PNGD_ADLER 65521u

// table entry of image `img` -> packet, geometry, inflate buffer (and with `out_bytes` >= 0 the output); false = PD_E_HEADER
__device__ static bool pngd_locate(const uint8_t* pk, const int32_t* table, int img, long pk_bytes, long infl_bytes, long out_bytes,
                                   PdGeom* g, long* poff, long* ioff, long* ooff) {
    const int32_t* te = table + 4 * (long)img;
    *poff = te[0]; *ioff = te[1]; *ooff = te[2];
    if (*poff < 0 || (*poff & 15) || *poff >= pk_bytes) return false;
    if (!pd_header(pk + *poff, pk_bytes - *poff, g)) return false;
    if (*ioff < 0 || (*ioff & 15) || *ioff + (long)g->inflated > infl_bytes) return false;
    if (out_bytes >= 0) {
        const long need = (long)g->H * g->W * g->channels;
        if (*ooff < 0 || *ooff + need > out_bytes) return false;
    }
    return true;
}

extern "C" __global__ __launch_bounds__(64) void png_inflate_kernel(const uint8_t* __restrict__ pk, const int32_t* __restrict__ table,
                                                                     uint8_t* infl, int32_t* __restrict__ status, long pk_bytes, long infl_bytes) {
    __shared__ PdTable lt, dt;
    __shared__ PdTok q[PNGD_QUEUE];
    __shared__ uint8_t lens[320];
    __shared__ long loc[2];
    __shared__ uint32_t ctl[4];
    const int img = blockIdx.x, lane = threadIdx.x;
    int32_t* st = status + 4 * (long)img;
    PdState s;                                    // used by lane 0 only
    PdGeom g;
    if (lane == 0) {
        long poff, ioff, ooff;
        const bool ok = pngd_locate(pk, table, img, pk_bytes, infl_bytes, -1, &g, &poff, &ioff, &ooff);
        ctl[2] = ok ? 1u : 0u;
        if (ok) {
            loc[0] = poff; loc[1] = ioff;
            ctl[3] = g.inflated;
            pd_init(&s, pk + poff + PD_HDR_BYTES, g.stream, g.inflated);
        } else {
            st[0] = PD_E_HEADER; st[1] = 0; st[2] = 0; st[3] = 0;
        }
    }
    __syncthreads();
    if (!ctl[2]) return;
    const uint8_t* stream = pk + loc[0] + PD_HDR_BYTES;
    uint8_t* out = infl + loc[1];
    const uint32_t out_len = ctl[3];
    for (;;) {
        if (lane == 0) {
            int n = 0, r = PD_R_TOKEN;
            while (n < PNGD_QUEUE) {
                r = pd_next(&s, &lt, &dt, lens, &q[n]);
                if (r != PD_R_TOKEN) break;
                ++n;
            }
            ctl[0] = (uint32_t)n;
            ctl[1] = r == PD_R_TOKEN ? 0u : (uint32_t)r;
        }
        __syncthreads();
        const int n = (int)ctl[0];
        const uint32_t fin = ctl[1];
        if (n > 0) {
            uint32_t vis = q[0].pos;              // output bytes below `vis` were stored before the last barrier
            for (int t = lane; t < n; t += 64)
                if (q[t].kind == PD_TOK_LITERAL) out[q[t].pos] = (uint8_t)q[t].arg;
            for (int t = 0; t < n; ++t) {
                const PdTok tok = q[t];
                if (tok.kind == PD_TOK_MATCH) {
                    const uint32_t dist = tok.arg, src0 = tok.pos - dist, span = tok.len < dist ? tok.len : dist;
                    if (src0 + span > vis) {
                        __syncthreads();
                        vis = tok.pos;
                    }
                    for (uint32_t k = lane; k < tok.len; k += 64) out[tok.pos + k] = out[src0 + (k < dist ? k : k % dist)];
                } else if (tok.kind == PD_TOK_STORED) {
                    for (uint32_t k = lane; k < tok.len; k += 64) out[tok.pos + k] = stream[tok.arg + k];
                }
            }
        }
        __syncthreads();
        if (fin) break;
    }
    if (lane == 0) ctl[0] = s.err;
    __syncthreads();
    uint32_t err = ctl[0];
    uint64_t S = 0, T = 0;
    if (!err) {                                   // (uniform) Adler-32 of the out_len bytes
        for (uint32_t i = lane; i < out_len; i += 64) {
            const uint32_t b = out[i];
            S += b;
            T += (uint64_t)(out_len - i) * b;     // < 2^63 summed over a lane's share of any out_len < 2^31
        }
        S %= PNGD_ADLER;
        T %= PNGD_ADLER;
        for (int o = 32; o > 0; o >>= 1) {
            S += __shfl_xor((unsigned long long)S, o, 64);
            T += __shfl_xor((unsigned long long)T, o, 64);
        }
    }
    if (lane == 0) {
        if (!err) {
            const uint32_t A = (uint32_t)((1 + S) % PNGD_ADLER), B = (uint32_t)((out_len + T) % PNGD_ADLER);
            if ((B << 16 | A) != s.adler) err |= PD_E_ADLER;
        }
        st[0] = (int32_t)err; st[1] = (int32_t)s.pos; st[2] = (int32_t)s.blocks; st[3] = (int32_t)s.tokens;
    }
}

extern "C" __global__ __launch_bounds__(64) void png_unfilter_kernel(const uint8_t* __restrict__ pk, const int32_t* __restrict__ table,
                                                                      const uint8_t* __restrict__ infl, uint8_t* __restrict__ outbuf,
                                                                      int32_t* __restrict__ status, long pk_bytes, long infl_bytes, long out_bytes) {
    __shared__ uint8_t rows[2][PD_MAX_ROWBYTES];
    __shared__ long loc[2];
    __shared__ int geo[8];
    const int img = blockIdx.x, lane = threadIdx.x;
    int32_t* st = status + 4 * (long)img;
    if (lane == 0) {
        PdGeom g;
        long poff, ioff, ooff;
        int ok = st[0] == 0;
        if (ok && !pngd_locate(pk, table, img, pk_bytes, infl_bytes, out_bytes, &g, &poff, &ioff, &ooff)) {
            st[0] = PD_E_HEADER;
            ok = 0;
        }
        geo[0] = ok;
        if (ok) {
            loc[0] = ioff; loc[1] = ooff;
            geo[1] = g.W; geo[2] = g.H; geo[3] = g.depth; geo[4] = g.channels; geo[5] = g.rowbytes;
        }
    }
    __syncthreads();
    if (!geo[0]) return;
    const int W = geo[1], H = geo[2], depth = geo[3], bpp = geo[4], rb = geo[5];       // (bpp: 3 for RGB, else 1 -- also on packed bytes)
    const uint8_t* in = infl + loc[0];
    uint8_t* out = outbuf + loc[1];
    for (int i = lane; i < rb; i += 64) rows[1][i] = 0;                               // the row above the first is zero
    __syncthreads();
    for (int y = 0; y < H; ++y) {
        uint8_t* cur = rows[y & 1];
        const uint8_t* prev = rows[(y & 1) ^ 1];
        const uint8_t* src = in + (long)y * (rb + 1);
        const int ft = src[0];
        for (int i = lane; i < rb; i += 64) cur[i] = src[1 + i];
        __syncthreads();
        if (ft > 4) {                                                                 // (uniform)
            if (lane == 0) st[0] = PD_E_FILTER;
            return;
        }
        if (ft == 2) {
            for (int i = lane; i < rb; i += 64) cur[i] = (uint8_t)(cur[i] + prev[i]);
        } else if (ft == 1) {
            // inclusive scan per channel over 64 bytes at a time; the carry of lane l is the last scanned value of its channel in the
            // chunk before: lane 63 - ((bpp - (l + 1) % bpp) % bpp)
            const int d = (lane + 1) % bpp, from = 63 - ((bpp - d) % bpp);
            uint32_t last = 0;
            for (int base = 0; base < rb; base += 64) {
                const int i = base + lane;
                uint32_t v = i < rb ? cur[i] : 0u;
                for (int o = bpp; o < 64; o <<= 1) {
                    const uint32_t t = __shfl_up(v, o, 64);
                    if (lane >= o) v += t;
                }
                v = (v + __shfl(last, from, 64)) & 255u;
                if (i < rb) cur[i] = (uint8_t)v;
                last = v;
            }
        } else if (ft != 0 && lane == 0) {
            for (int i = 0; i < rb; ++i) {
                const int a = i >= bpp ? cur[i - bpp] : 0, b = prev[i], c = i >= bpp ? prev[i - bpp] : 0;
                cur[i] = (uint8_t)(cur[i] + (ft == 3 ? ((a + b) >> 1) : pd_paeth(a, b, c)));
            }
        }
        __syncthreads();
        if (depth == 8) {
            uint8_t* dst = out + (long)y * rb;
            for (int i = lane; i < rb; i += 64) dst[i] = cur[i];
        } else {
            uint8_t* dst = out + (long)y * W;
            const int mask = (1 << depth) - 1;
            for (int x = lane; x < W; x += 64) {
                const int bit = x * depth;
                dst[x] = (uint8_t)((cur[bit >> 3] >> (8 - depth - (bit & 7))) & mask);
            }
        }
    }
}

// RESIZE flags 64 / 128 (slots: include/cutie_hip.h, ABI 11, forms added)
int launch_png_decode(const cutie_op* op, hipStream_t s) {
    const uint64_t* p = op->p;
    const int N = op->i[0];
    const long pk_bytes = op->i[1], infl_bytes = op->i[2], out_bytes = op->i[3];
    if (op->flags & ~192) { cutie_set_error("png decode: flags 64 / 128 cannot be combined with other RESIZE flags (%d)", op->flags); return -2; }
    if (N < 1 || N > 65535) { cutie_set_error("png decode: %d images, 1 .. 65535", N); return -2; }
    if (pk_bytes < 0 || infl_bytes < 0 || out_bytes < 0) { cutie_set_error("png decode: negative buffer size"); return -2; }
    const bool unf = op->flags & 128;
    if (!p[0] || !p[1] || !p[2] || !p[4] || (unf && !p[3])) {
        cutie_set_error("png decode: needs the packets (p0), the table (p1), the inflate buffer (p2), the status (p4)%s", unf ? " and the output (p3)" : "");
        return -2;
    }
    if ((p[0] & 15) || (p[1] & 15) || (p[2] & 15) || (p[4] & 15)) { cutie_set_error("png decode: packets, table, inflate buffer and status 16-byte aligned"); return -2; }
    if (op->flags & 64)
        hipLaunchKernelGGL(png_inflate_kernel, dim3(N), dim3(64), 0, s, (const uint8_t*)p[0], (const int32_t*)p[1], (uint8_t*)p[2], (int32_t*)p[4],
                           pk_bytes, infl_bytes);
    if (unf)
        hipLaunchKernelGGL(png_unfilter_kernel, dim3(N), dim3(64), 0, s, (const uint8_t*)p[0], (const int32_t*)p[1], (const uint8_t*)p[2],
                           (uint8_t*)p[3], (int32_t*)p[4], pk_bytes, infl_bytes, out_bytes);
    return (int)hipGetLastError();
}
