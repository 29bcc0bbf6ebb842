// The wave-level parts that the two PNG encoders (png.hip, png_photo.hip) share, on top of the scalar core deflate_enc_core.h: run lengths
// over ballot masks, the scan of the rows' bit counts with the zlib framing and the status block, and the shift of a row's bits to its
// offset in the stream.  Device only; include after common.h.
// (jpeg_enc.hip is not a user: it writes MSB-first into big-endian words and scans to 64-bit offsets -- other helpers, not these with flags.)
#ifndef CUTIE_DEFLATE_ENC_H
#define CUTIE_DEFLATE_ENC_H

#include "deflate_enc_core.h"

// number of set bits of `mask` from bit i on, counted up to CAP (0: to the end).  The masks are zero from bit L on and mask[nmask] is a
// zero word, so a run ends inside the row and a shift by i & 63 of the last mask word never needs a word behind it.
template <int CAP>
__device__ __forceinline__ int de_run(const uint64_t* mask, int i, int nmask) {
    int k = i >> 6;
    uint64_t z = ~mask[k] >> (i & 63);             // (the shifted-in zeros of ~mask are ones of mask only beyond bit 63: handled below)
    if (z) return CAP ? min(__builtin_ctzll(z), CAP) : __builtin_ctzll(z);
    int pos = (k + 1) << 6;
    for (++k; k <= nmask && (!CAP || pos - i < CAP); ++k, pos += 64) {
        z = ~mask[k];
        if (z) return CAP ? min(pos + __builtin_ctzll(z) - i, CAP) : pos + __builtin_ctzll(z) - i;
    }
    return CAP ? min(pos - i, CAP) : pos - i;
}

// The body of a scan kernel: one block of 1024.  info[r] = {bits, sum of the row's bytes mod 65521, sum of (L - j) * byte_j mod 65521, -}
// of H rows of L bytes; info[r].w becomes the row's exclusive bit offset behind the `front` constant bits of the stream.  Adler-32 of the
// whole image from the partials (Adler composes: all sums are integers mod 65521, so the order of the additions does not matter), length
// check against the capacity, then exactly the words the stream will use are cleared and word 0 and the trailer are written; `back`
// constant bits follow the rows.  status = {stream bytes, Adler-32, error bits (1: the stream does not fit the capacity; nothing is
// written then), 0}
__device__ __forceinline__ void de_scan(int4* __restrict__ info, int H, int L, uint32_t front, uint32_t back, uint32_t word0,
                                        uint8_t* __restrict__ out, int cap, int* __restrict__ status) {
    __shared__ uint32_t part[1024];
    __shared__ uint64_t red[2][16];
    __shared__ uint32_t carry_s, len_s;
    const int t = threadIdx.x;
    if (t == 0) carry_s = 0;
    __syncthreads();
    uint64_t a = 0, bsum = 0;
    for (int base = 0; base < H; base += 1024) {
        const int r = base + t;
        const int4 v = r < H ? info[r] : make_int4(0, 0, 0, 0);
        part[t] = (uint32_t)v.x;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {                     // inclusive scan of the 1024 bit counts
            const uint32_t add = t >= o ? part[t - o] : 0u;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        const uint32_t carry = carry_s;
        if (r < H) {
            info[r].w = (int)(carry + part[t] - (uint32_t)v.x);
            a += (uint32_t)v.y;
            bsum += ((uint64_t)(H - 1 - r) * L % DE_ADLER) * (uint32_t)v.y % DE_ADLER + (uint32_t)v.z;
        }
        __syncthreads();
        if (t == 1023) carry_s = carry + part[1023];
        __syncthreads();
    }
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor((unsigned long long)a, o, 64);
        bsum += __shfl_xor((unsigned long long)bsum, o, 64);
    }
    if ((t & 63) == 0) { red[0][t >> 6] = a; red[1][t >> 6] = bsum; }
    __syncthreads();
    if (t == 0) {
        uint64_t A = 1, B = (uint64_t)H * L % DE_ADLER;
        for (int k = 0; k < 16; ++k) { A += red[0][k] % DE_ADLER; B += red[1][k] % DE_ADLER; }
        const uint32_t adler = (uint32_t)(B % DE_ADLER) << 16 | (uint32_t)(A % DE_ADLER);
        const uint32_t body = (front + carry_s + back + 7u) >> 3, len = body + 4u;       // then 4 bytes Adler-32
        const bool fits = len <= (uint32_t)cap;
        status[0] = (int)len;
        status[1] = (int)adler;
        status[2] = fits ? 0 : 1;
        status[3] = 0;
        len_s = fits ? len : 0u;
        red[0][0] = adler;
    }
    __syncthreads();
    const uint32_t len = len_s;
    if (len == 0) return;
    uint32_t* w = (uint32_t*)out;
    const uint32_t nw = (len + 3) >> 2;                           // cap is a multiple of 4 (launch check): within the buffer
    for (uint32_t k = t; k < nw; k += 1024) w[k] = 0u;
    __syncthreads();
    if (t == 0) {
        w[0] = word0;
        const uint32_t adler = (uint32_t)red[0][0];
        for (int k = 0; k < 4; ++k) out[len - 4 + k] = (uint8_t)(adler >> (24 - 8 * k));
    }
}

// One wave: the image src[0 .. nsrc) of nbits > 0 bits goes to bit offset `off` of the cleared stream.  Interior words have one owner (plain
// stores); the first and the last word are shared with the neighbours and are OR-ed in with a vector atomic.
__device__ __forceinline__ void de_shift_out(const uint32_t* src, uint32_t nsrc, uint32_t nbits, uint32_t off, uint32_t* __restrict__ out, int lane) {
    const uint32_t w0 = off >> 5, w1 = (off + nbits - 1) >> 5, sh = off & 31u;
    for (uint32_t k = lane; k <= w1 - w0; k += 64) {
        const uint32_t lo = k < nsrc ? src[k] : 0u, prev = (k > 0 && k - 1 < nsrc) ? src[k - 1] : 0u;
        const uint32_t val = sh ? (lo << sh) | (prev >> (32 - sh)) : lo;
        if (k == 0 || k == w1 - w0) atomicOr(out + w0 + k, val);
        else out[w0 + k] = val;
    }
}

#endif
