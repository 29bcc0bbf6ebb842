// STEM: the first three launches of the ResNet encoders in one -- IMG_PREP (normalise, pad, attach mask / others planes), the 7x7 /
// stride-2 / pad-3 convolution with folded BatchNorm (pixel_encoder.conv1, mask_encoder.conv1: resnet.py conv1 + bn1; big_modules.py
// 30-33, 95-100) and the 3x3 / stride-2 / pad-1 max pooling (+ ReLU: before the pool in the pixel encoder, after it in the mask
// encoder -- the same thing, ReLU and max commute).  Round 2 ran them as three launches through two HBM round trips of a stride-2 map
// (480p: 30.4 + 10.2 + 6.6 us per frame, the 7x7 conv at 2.6 % of the MFMA peak: Cin = 3 padded to 8, register-staged im2col);
// this kernel: 13.5 us (4 x 16 tiles with per-wave weight loads: 24 us; weights staged once per block: 17.7; 8 x 16 tiles, one round: 13.5).
//
// One block = ST_PH x 16 pooled pixels of one object (8 x 16: they need 17 x 33 conv pixels, which need a 39 x 71 input patch; 210 blocks
// at 480p: one round on 256 CUs).
//   1. the patch is built in LDS as [39][72] pixels x 8 bf16 channels (r, g, b, mask, others, 0, 0, 0), straight from the fp32 frame;
//      pixels outside the padded frame are the conv's zero padding, the 72nd column is zero (the 8th "tap" of a row, see below);
//   2. implicit GEMM on v_mfma_f32_16x16x32_bf16: a K step is half a kernel row = 4 taps x 8 channels, so a B fragment is ONE
//      16-byte LDS read of the pixel the tap lands on (lane group g <-> tap 4 (s & 1) + g; the 8th tap has zero weights); A = the
//      weights (staged once per block in LDS in fragment order, then 2 x 14 fragments per wave in registers); 8 waves = 4 (pixel groups) x 2 (channel halves);
//   3. bias (+ nothing else: ReLU moves behind the pool), bf16, into an LDS tile [561][64] that aliases the patch; conv pixels outside
//      the conv's output range are written as -inf (the pool's padding);
//   4. 3 x 3 max over the tile, ReLU, 32-byte stores.
// Results: identical rounding points as the three-launch form (bf16 after the conv, max of bf16 values); only the fp32 summation
// order inside the conv differs.
#include "common.h"
#include <math.h>

#ifndef ST_PH
#define ST_PH 8
#endif
#define ST_PW 16
#define ST_CH (2 * ST_PH + 1)                            // conv rows of a block
#define ST_CW (2 * ST_PW + 1)                            // conv columns (33)
#define ST_NCONV (ST_CH * ST_CW)
#define ST_MF ((ST_NCONV + 15) / 16)                     // M fragments
#define ST_IH (2 * ST_CH + 5)                            // input rows
#define ST_IW 72                                         // input columns: 71 + one zero column
#define ST_CLD 72                                        // bf16 pitch of the conv tile (64 + 8: rows 144 B apart)

typedef __attribute__((ext_vector_type(4))) unsigned int st_u4;

#define ST_MAXIMG 12
struct StemParams {
    const float* img; const float* masks; const bf16_t* W; const float* bias; bf16_t* y;
    int h0, w0, H, W_, pl, pt, K, Kpad, relu, gx, nb;
    float m0, m1, m2, s0, s1, s2;
    // ABI 4: several frames per launch (grid.y): frame f > 0 reads imgs[f - 1] (f = 0: img), masks + f * mstride floats and writes
    // y + f * K * (H/4) * (W/4) * 64 -- the look-ahead window of the image encoder / the clips of a lock-step group in ONE round-filling launch
    const float* imgs[ST_MAXIMG - 1]; long mstride;
    // mixed form (clips in lock step with different object counts): the clips' counts as 3-bit fields (common.h); frame f = clip f has
    // K_f objects, its masks lie (start_f + f) planes behind p.masks and its output start_f objects behind p.y; grid.z = the largest count
    unsigned counts;
};

#define ST_NT 512                                        // 8 waves: 4 pixel groups x 2 channel halves (two waves per SIMD hide each other's LDS latency)
#define STEM_KERNEL_NAME stem_kernel
#define STEM_MIXED false
#include "stem_body.h"
#undef STEM_KERNEL_NAME
#undef STEM_MIXED
#define STEM_KERNEL_NAME stem_mixed_kernel
#define STEM_MIXED true
#include "stem_body.h"
#undef STEM_KERNEL_NAME
#undef STEM_MIXED

int launch_stem(const cutie_op* op, hipStream_t s) {
    const int32_t* i = op->i;
    const uint64_t* q = op->p;
    if (!q[0] || !q[2] || !q[3] || !q[4]) { cutie_set_error("stem: image, packed weights, bias and output required"); return -2; }
    if ((i[2] & 15) || (i[3] & 15) || i[6] < 1 || i[7] < 392 || (i[7] & 7)) {
        cutie_set_error("stem: H, W multiples of 16, K >= 1, Kpad >= 392 (H=%d W=%d K=%d Kpad=%d)", i[2], i[3], i[6], i[7]);
        return -2;
    }
    StemParams p;
    p.img = (const float*)q[0]; p.masks = (const float*)q[1]; p.W = (const bf16_t*)q[2]; p.bias = (const float*)q[3]; p.y = (bf16_t*)q[4];
    p.h0 = i[0]; p.w0 = i[1]; p.H = i[2]; p.W_ = i[3]; p.pl = i[4]; p.pt = i[5]; p.K = q[1] ? i[6] : 1; p.Kpad = i[7]; p.relu = op->flags & 1;
    p.m0 = op->f[0]; p.m1 = op->f[1]; p.m2 = op->f[2]; p.s0 = op->f[3]; p.s1 = op->f[4]; p.s2 = op->f[5];
    const int PH = i[2] >> 2, PW = i[3] >> 2;
    p.gx = (PW + ST_PW - 1) / ST_PW;
    p.nb = p.gx * ((PH + ST_PH - 1) / ST_PH);
    constexpr size_t lds = ST_MF * 16 * ST_CLD * 2 + 4 * 14 * 64 * 16;
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(stem_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void*>(stem_mixed_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            cutie_set_error("stem: cannot raise the dynamic LDS limit to %d bytes", (int)lds);
            return -2;
        }
        attr_set = true;
    }
    int nimg = i[8] > 1 ? i[8] : 1;                      // frames per launch: image f > 0 at p[4 + f] (p5 .. p15), masks i9 floats apart
    if (nimg > ST_MAXIMG) { cutie_set_error("stem: at most %d frames per launch (%d)", ST_MAXIMG, nimg); return -2; }
    p.mstride = i[9];
    for (int f = 1; f < ST_MAXIMG; ++f) {
        p.imgs[f - 1] = f < nimg ? (const float*)q[4 + f] : nullptr;
        if (f < nimg && !q[4 + f]) { cutie_set_error("stem: frame %d of %d has no image", f, nimg); return -2; }
    }
    p.counts = 0;
    if (i[10]) {                                         // mixed form: i10 = the counts of the i8 clips, i6 = the largest of them; i9 unused (the masks are dense planes)
        int objs; const int nc = mixed_clips((unsigned)i[10], &objs);
        int kmax = 0;
        for (int c = 0; c < nc; ++c) kmax = mixed_count((unsigned)i[10], c) > kmax ? mixed_count((unsigned)i[10], c) : kmax;
        if (nc < 1 || nc != nimg || !q[1] || kmax != i[6]) { cutie_set_error("stem (mixed form): %d clips in the counts 0x%x, %d frames; needs masks and K = the largest count", nc, i[10], nimg); return -2; }
        p.counts = (unsigned)i[10];
        hipLaunchKernelGGL(stem_mixed_kernel, dim3(((p.nb + 7) / 8) * 8, nimg, p.K), dim3(ST_NT), lds, s, p);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(stem_kernel, dim3(((p.nb + 7) / 8) * 8, nimg, p.K), dim3(ST_NT), lds, s, p);
    return (int)hipGetLastError();
}
