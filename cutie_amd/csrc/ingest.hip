// Frame ingest (ABI 5): RESIZE with flags&2 (antialiased bilinear, torch's _upsample_bilinear2d_aa) and / or flags&4 (uint8
// interleaved source, ToTensor).  The decoded frame arrives as u8 [H, W, C] (what PIL / numpy decode) and leaves as the f32
// [C, OH, OW] frame the host path builds with ToTensor + F.interpolate(antialias=True); see the RESIZE block of
// include/cutie_hip.h for the contract and DESIGN.md section 5 for the numerics.
//
// The tap table (first tap, tap count, normalised weights per output column and row) is built on the host, once per
// geometry (cutie_amd/ops.py aa_taps): torch rounds center / support / weights through a mix of fp32 and fp64 steps, which is
// simplest to mirror in one place, and the table is a few KB.  The kernels only read it, clamped to the source extent.
//
// Two passes as torch runs them: horizontal (source -> f32 scratch [C, H, OW]), then vertical (scratch -> dst), taps summed in
// ascending order, product then add (-ffp-contract=off).  One thread per output quad (4 adjacent columns), all channels.
#include "common.h"

#define GRID1D(n, bs) dim3((unsigned)(((long)(n) + (bs) - 1) / (bs)))

// u8 -> f32 exactly as u8.float().div_(255.0): a correctly rounded fp32 division (HIP's default fp32 '/')
__device__ __forceinline__ float u8f(uint32_t b) { return (float)b / 255.0f; }

// pure ToTensor: u8 [H, W, C] (row stride sld bytes, pixel stride C) -> f32 [C, H, W]
__global__ void u8_to_f32_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int C, int H, int W, long sld) {
    const int nq = (W + 3) >> 2;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)H * nq) return;
    const int y = (int)(idx / nq), x0 = (int)(idx - (long)y * nq) * 4;
    const uint8_t* row = src + (long)y * sld + (long)x0 * C;
    const bool full = x0 + 4 <= W;
    const long plane = (long)H * W;
    float* out = dst + (long)y * W + x0;
    if (C == 3 && full && ((uintptr_t)row & 3) == 0) {
        // 12 bytes = the 4 pixels' RGB triples in three dword loads
        const uint32_t w0 = ((const uint32_t*)row)[0], w1 = ((const uint32_t*)row)[1], w2 = ((const uint32_t*)row)[2];
        const uint32_t b[12] = {w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255, w0 >> 24, w1 & 255, (w1 >> 8) & 255,
                                (w1 >> 16) & 255, w1 >> 24, w2 & 255, (w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float4 v = make_float4(u8f(b[c]), u8f(b[3 + c]), u8f(b[6 + c]), u8f(b[9 + c]));
            if ((W & 3) == 0) *(float4*)(out + c * plane) = v;
            else { out[c * plane] = v.x; out[c * plane + 1] = v.y; out[c * plane + 2] = v.z; out[c * plane + 3] = v.w; }
        }
        return;
    }
    const int n = full ? 4 : W - x0;
    for (int c = 0; c < C; ++c)
        for (int k = 0; k < n; ++k) out[c * plane + k] = u8f(row[k * C + c]);
}

// horizontal pass: src (u8 [H, W, C] row stride sld bytes | f32 planes, plane stride splane, row stride sld elements)
// -> tmp f32 [C, H, OW].  tab: OW rows of K2 = 2 + K words (first, count, K fp32 weights as bits)
template <bool U8>
__global__ void resize_aa_h_kernel(const void* __restrict__ src, float* __restrict__ tmp, const int* __restrict__ tab, int K2,
                                   int C, int H, int W, int OW, long splane, long sld) {
    const int nq = (OW + 3) >> 2;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)H * nq) return;
    const int y = (int)(idx / nq), x0 = (int)(idx - (long)y * nq) * 4;
    const int n = min(4, OW - x0);
    int first[4], count[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int* t = tab + (long)min(x0 + k, OW - 1) * K2;
        first[k] = min(max(t[0], 0), W - 1);
        count[k] = k < n ? min(t[1], min(K2 - 2, W - first[k])) : 0;
    }
    for (int c = 0; c < C; ++c) {
        float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float* w = (const float*)(tab + (long)(x0 + min(k, n - 1)) * K2 + 2);
            float acc = 0.f;
            for (int j = 0; j < count[k]; ++j) {
                const int x = first[k] + j;
                const float v = U8 ? u8f(((const uint8_t*)src)[(long)y * sld + (long)x * C + c])
                                   : ((const float*)src)[(long)c * splane + (long)y * sld + x];
                acc = j == 0 ? v * w[0] : acc + v * w[j];
            }
            o[k] = acc;
        }
        float* out = tmp + ((long)c * H + y) * OW + x0;
        if ((OW & 3) == 0) *(float4*)out = make_float4(o[0], o[1], o[2], o[3]);
        else for (int k = 0; k < n; ++k) out[k] = o[k];
    }
}

// vertical pass: tmp f32 [C, H, OW] -> dst f32 [C, OH, OW].  tab: OH rows of K2 words
__global__ void resize_aa_v_kernel(const float* __restrict__ tmp, float* __restrict__ dst, const int* __restrict__ tab, int K2,
                                   int C, int H, int OH, int OW) {
    const int nq = (OW + 3) >> 2;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)C * OH * nq) return;
    const int q = (int)(idx % nq);
    const long r = idx / nq;
    const int oy = (int)(r % OH), c = (int)(r / OH), x0 = q * 4;
    const int n = min(4, OW - x0);
    const int* t = tab + (long)oy * K2;
    const int first = min(max(t[0], 0), H - 1), count = min(t[1], min(K2 - 2, H - first));
    const float* w = (const float*)(t + 2);
    const float* in = tmp + ((long)c * H + first) * OW + x0;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < count; ++j) {
        float4 v;
        if ((OW & 3) == 0) v = *(const float4*)(in + (long)j * OW);
        else {
            const float* p = in + (long)j * OW;
            v = make_float4(p[0], n > 1 ? p[1] : 0.f, n > 2 ? p[2] : 0.f, n > 3 ? p[3] : 0.f);
        }
        const float wj = w[j];
        if (j == 0) acc = make_float4(v.x * wj, v.y * wj, v.z * wj, v.w * wj);
        else acc = make_float4(acc.x + v.x * wj, acc.y + v.y * wj, acc.z + v.z * wj, acc.w + v.w * wj);
    }
    float* out = dst + ((long)c * OH + oy) * OW + x0;
    if ((OW & 3) == 0) *(float4*)out = acc;
    else {
        const float a[4] = {acc.x, acc.y, acc.z, acc.w};
        for (int k = 0; k < n; ++k) out[k] = a[k];
    }
}

int launch_resize_ingest(const cutie_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    const uint64_t* p = op->p;
    const int BS = 256;
    const int C = i[0], H = i[1], W = i[2], OH = i[3], OW = i[4];
    const bool aa = op->flags & 2, u8 = op->flags & 4;
    if (C < 1 || H < 1 || W < 1 || OH < 1 || OW < 1) { cutie_set_error("resize: empty shape"); return -2; }
    if (op->flags & 1) { cutie_set_error("resize: nearest (flags&1) cannot be combined with flags&2 / flags&4"); return -2; }
    if (!p[0] || !p[1]) { cutie_set_error("resize: null source or destination"); return -2; }
    if (u8 && i[6] < W * C) { cutie_set_error("resize: u8 row stride %d < W*C = %d", i[6], W * C); return -2; }
    if (((uintptr_t)p[1] & 15) != 0) { cutie_set_error("resize: flags&2 / flags&4 need a 16-byte aligned destination"); return -2; }
    if (!aa) {
        if (OH != H || OW != W) { cutie_set_error("resize: flags 4 alone is ToTensor, needs OH == H and OW == W"); return -2; }
        hipLaunchKernelGGL(u8_to_f32_kernel, GRID1D((long)H * ((W + 3) / 4), BS), dim3(BS), 0, s, (const uint8_t*)p[0], (float*)p[1],
                           C, H, W, (long)i[6]);
        return (int)hipGetLastError();
    }
    const int K2 = i[7] + 2;
    if (!p[2] || !p[3] || i[7] < 1) { cutie_set_error("resize: antialias needs the tap table (p2, i7 >= 1) and the scratch (p3)"); return -2; }
    if (((uintptr_t)p[3] & 15) != 0) { cutie_set_error("resize: antialias needs a 16-byte aligned scratch"); return -2; }
    const int* tab = (const int*)p[2];
    const long nh = (long)H * ((OW + 3) / 4);
    if (u8)
        hipLaunchKernelGGL(resize_aa_h_kernel<true>, GRID1D(nh, BS), dim3(BS), 0, s, (const void*)p[0], (float*)p[3], tab, K2,
                           C, H, W, OW, 0L, (long)i[6]);
    else
        hipLaunchKernelGGL(resize_aa_h_kernel<false>, GRID1D(nh, BS), dim3(BS), 0, s, (const void*)p[0], (float*)p[3], tab, K2,
                           C, H, W, OW, (long)i[5], (long)i[6]);
    hipLaunchKernelGGL(resize_aa_v_kernel, GRID1D((long)C * OH * ((OW + 3) / 4), BS), dim3(BS), 0, s, (const float*)p[3], (float*)p[1],
                       tab + (long)OW * K2, K2, C, H, OH, OW);
    return (int)hipGetLastError();
}
