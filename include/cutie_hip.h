/*
 * cutie_hip.h -- C ABI of libcutie_hip.so, the MI355X (gfx950) kernel library behind the
 * Cutie per-frame inference hot path (InferenceCore.step).
 *
 * The reference (hkchengrex/Cutie) has no FFI for this path: all arithmetic is delegated to
 * torch ops.  This header is therefore the boundary WE define under the
 * reference's Python surface (cutie.model.cutie.CUTIE / cutie.inference.inference_core.InferenceCore,
 * mirrored in cutie_amd/).  Each op below cites the reference torch-op sequence it replaces.
 *
 * Conventions
 *   - plain C, no torch types: raw device pointers + explicit sizes; the caller owns all memory
 *     (nothing is allocated inside); every entry point takes the hipStream_t to launch on (as void*).
 *   - return 0 on success, negative on error; cutie_hip_last_error() gives the message.
 *   - activations are NHWC ("pixel-major, channel-contiguous") bf16 unless stated; batch = objects.
 *   - a frame is executed as a *launch plan*: an array of cutie_op descriptors over a pre-allocated
 *     arena, replayed by cutie_exec() (one C call per stage; graph-capturable: no allocation, no sync).
 */
#ifndef CUTIE_HIP_H
#define CUTIE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CUTIE_OP_NI 24
#define CUTIE_OP_NF 6
#define CUTIE_OP_NP 16
#define CUTIE_MERGE_MAX_SOURCES 8   /* PROB_TO_ID flags&16 (ABI 8) */
#define CUTIE_PNG_PHOTO_ROW_LIMIT 16384   /* PROB_TO_ID flags == 16384 (ABI 11, form added): filtered bytes per row, W * B + 1 */
#define CUTIE_GUIDED_MAX_RADIUS 64  /* PROB_TO_ID flags == 32768 (ABI 11, form added): the largest window radius */
#define CUTIE_GUIDED_MAX_PLANES 16  /* ... planes per op; the host splits more over several ops */
#define CUTIE_REDACT_MAX_RADIUS 64  /* PROB_TO_ID flags == 65536 (ABI 11, form added): the largest blur radius */
#define CUTIE_REDACT_MAX_CELL 256   /* ... the largest pixelate cell */
#define CUTIE_EDT_MAX_LIMIT 65536   /* PROB_TO_ID flags == 4096 (ABI 11, form added): distances are exact below it; radii up to 255 (255^2 = 65025) */
#define CUTIE_EDT_MAX_SETS 16       /* ... sets of ids per op; the host splits more over several ops */
#define CUTIE_JF_MAX_RADIUS 40      /* PROB_TO_ID flags == 64 (ABI 10): the largest match radius; 2160 x 3840 needs 36 */

/* Mixed forms (added without a new ABI number: cutie_hip_build_flags() bit 3, value 8, says they are present -- a library from before
 * would ignore the counts word and run the uniform form, so the callers ask first: cutie_amd/_lib.py has_mixed_lockstep).
 * Clips in lock step (ABI 4) used to hold the same number of objects each, and every launch that couples the objects of a clip found the
 * clip of object b as b / objects_per_clip.  In a MIXED group clip c holds K_c objects, 1 <= K_c <= 7, at most 8 clips.  The counts
 * travel as ONE 24-bit word of 3-bit fields -- clip c at bits 3c .. 3c + 2, a zero field ends the list -- in an integer slot that every
 * uniform descriptor leaves 0 (no device table: the word is a kernel argument, and every offset a launch needs is a prefix sum over at
 * most 8 fields, scalar arithmetic where the clip is block-uniform): start_c = K_0 + .. + K_(c-1) is clip c's first object, object b
 * belongs to the clip with start_c <= b < start_c + K_c.  Per-object tensors stay clip-major and dense (clip c's objects at start_c);
 * the probability tensor of a mixed group holds sum(K_c) + clips planes, clip c's K_c + 1 planes from plane start_c + c on.
 * The forms: UPSAMPLE2X_ADD i6, UP4_SOFTMAX i5, ATTN_Q2P (chain form) i10, STEM i10, COPY2D i4 -- see each op.  The uniform encodings keep
 * their meaning bit for bit and reach the same kernel instantiations (the launchers branch on the word).  CONV has no mixed form: the
 * per-clip broadcast residual (f0 / f1) of a mixed group is expanded to one map per object by COPY2D i4 and added as an ordinary
 * residual -- the same values, the conv kernels untouched.  The joint AFF_READOUT (i8) has none either: a mixed group reads every bank
 * in its clip's own look-ahead lane.  Per clip every mixed launch computes exactly what the uniform launch of that clip alone computes. */
typedef struct cutie_op {
    int32_t kind;               /* CUTIE_OP_* */
    int32_t flags;              /* op-specific bit flags */
    int32_t i[CUTIE_OP_NI];     /* integer parameters (per-op meaning below) */
    float f[CUTIE_OP_NF];       /* float parameters */
    uint64_t p[CUTIE_OP_NP];    /* device pointers */
} cutie_op;                     /* 256 bytes, mirrored by cutie_amd/ops.py:OP_DTYPE */

/* ---- conv flags ---- */
#define CUTIE_F_RELU_IN   1   /* relu applied to the input while loading (conv(F.relu(x))) */
#define CUTIE_F_OUT_F32   2   /* output stored as f32 (default bf16) */
#define CUTIE_F_RES_BCAST 4   /* residual has batch 1 and is broadcast over the B objects */
#define CUTIE_F_PLAIN     8   /* A/B switch: the general kernel where a specialised one exists (Cout == 1 on large maps) */
#define CUTIE_F_TILE_OFF  128 /* A/B switch: Cout == 1, Cin == 128 on large maps without the LDS-tiled kernel (conv_cout1_tile_kernel) */
#define CUTIE_F_PRIO      256 /* the launch belongs to the frame's critical path (the caller's stream): its waves raise their issue priority
                               * (s_setprio 1), so that look-ahead work sharing the compute units (window encoder, stacked read-outs) fills
                               * the gaps instead of taking every other issue slot.  CONV, and since ABI 4 UPSAMPLE2X_ADD, AREA_DOWN3, ECA_APPLY,
                               * GRU (four-channel form), UP4_SOFTMAX (four-pixel forms) and the chain forms of ATTN_Q2P / ATTN_SELF / ATTN_P2Q / QFFN
                               * (ABI 3 raised it unconditionally there); AFF_SCORE / AFF_SELECT / AFF_READOUT use flags&64 */
#define CUTIE_ACT_SHIFT   4   /* activation code in bits 4..6 */
#define CUTIE_ACT_NONE    0
#define CUTIE_ACT_RELU    1
#define CUTIE_ACT_SIGMOID 2
#define CUTIE_ACT_SQ1     3   /* x*x + 1   (shrinkage, big_modules.py:84) */

enum {
    /* CONV: y = act(conv2d(relu_in?(cat(x1,x2)), w) + bias + res)   -- implicit-GEMM on MFMA.
     * replaces nn.Conv2d / GConv2d (+ folded BatchNorm2d + ReLU + residual add) everywhere:
     * resnet.py:51-124, big_modules.py:36,81-87,207-235,257-306, group_modules.py:33-58,102-127,
     * channel_attn.py:25-29, modules.py:22-31,46-85, nn.Linear on pixel tokens (object_transformer.py,
     * transformer_layers.py, object_summarizer.py).
     * p0=x1 bf16 [B,H,W,ldx1]  p1=x2 bf16 [B,H,W,ldx2] (virtual channel concat, may be 0)
     * p2=w bf16 [CoutPad][Kpad] (k = (kh*KW+kw)*Cin + c, zero padded)  p3=bias f32[Cout] (may be 0)
     * p4=res bf16 [B|1,OH,OW,ldr] (may be 0)  p5=y bf16|f32 [B,OH,OW,ldy]
     * i: 0 B 1 H 2 W 3 C1 4 C2 5 ldx1 6 ldx2 7 OH 8 OW 9 Cout 10 ldy 11 KH 12 KW 13 stride 14 pad
     *    15 ldr 16 Kpad 17 tile id (table in conv_igemm.hip launch_conv / cutie_amd/ops.py TILES; 19 = Cout==1 kernel)
     *    18 real (un-padded) input channels: ignored by the kernel, used for flop accounting
     *    19 split-K factor (<=1: none; must divide Kpad/BK of the chosen tile).  grid.z slices the K tiles, every slice
     *       parks its fp32 partial tile in p6 and a second launch sums the slices in slice order (deterministic) and
     *       runs the epilogue.  p6 = f32 scratch, capacity i20*1024 floats >= splitk*M*roundup(Cout,8).
     *    side jobs (LDS-DMA tiles only): p7 = int64 [B,Cout] GAP accumulator the stored output is added to (x 2^24: every stored VALUE is
     *       converted to fixed point before anything is summed, so the accumulator is the same integer for every tile and arrival order;
     *       exact for |value| <= 2^20, beyond that +-2^20 saturate and NaN counts 0: DESIGN.md section 5);
     *       p8 = int64 buffer of i21 words cleared by this launch.
     *    p9 / i22, p10 / i23 (producer / consumer tiles 100.., else ignored; 0 = none): device ranges [p, p + bytes) that the
     *       producer waves read and discard once their last DMA piece is out -- the packed weights of the following conv(s)
     *       of the list, so that they are in every XCD's L2 when that launch starts.  Never changes a result.
     *    ABI 4 -- clips in lock step (several independent clips through one launch, batch = clips x objects; the reference runs one
     *       InferenceCore per video, eval_vos.py:97): with CUTIE_F_RES_BCAST and f0 > 0 the B objects come in groups of (int)f0 -- one clip
     *       each -- and group q adds ITS residual map [OH,OW,ldr] at p4 + q * (int)f1 rows (f1 >= OH*OW, a whole number; what
     *       MainToGroupDistributor('add') broadcasts per clip, group_modules.py:61-99).  f0 = 0: one map for all objects, as before. */
    CUTIE_OP_CONV = 1,
    /* MAXPOOL 3x3 s2 p1 (+relu if flags&1): resnet.py:131-134, big_modules.py:47-48,158-160
     * p0=x bf16 [B,H,W,C] p1=y bf16 [B,OH,OW,C]   i: 0 B 1 H 2 W 3 C 4 OH 5 OW */
    CUTIE_OP_MAXPOOL = 2,
    /* IMG_PREP: (image-mean)/std, zero-pad to /16, CHW f32 -> NHWC8 bf16; with masks also the
     * per-object [image, mask_k, others_k] stack of the mask encoder.
     * cutie.py:62,76,49-59; tensor_utils.py:7-22; big_modules.py:134-139
     * p0=image f32 [3,h0,w0] p1=masks f32 [K,H,W] (0 => K=1, image only) p2=y bf16 [K,H,W,8]
     * i: 0 h0 1 w0 2 H 3 W 4 pad_left 5 pad_top 6 K     f: 0..2 mean 3..5 std */
    CUTIE_OP_IMG_PREP = 3,
    /* UPSAMPLE2X_ADD: y = bilinear_x2(g, align_corners=False) + skip (broadcast over objects)
     * group_modules.py:19-23 + MainToGroupDistributor('add') modules.py:15-18
     * p0=g bf16 [B,h,w,C] p1=skip bf16 [1,2h,2w,C] p2=y bf16 [B,2h,2w,C]   i: 0 B 1 h 2 w 3 C
     * ABI 4: i4 > 0 = objects per clip (clips in lock step, see CONV): group q = b / i4 adds the skip map at p1 + q * i5 pixels (i5 >= 4hw)
     * Mixed form: i6 != 0 = the clips' object counts (3-bit fields, sum = B; i4 = 0): object b adds the map of ITS clip, p1 + clip(b) * i5 pixels */
    CUTIE_OP_UPSAMPLE2X_ADD = 4,
    /* AREA_DOWN: r x r mean (F.interpolate mode='area', integer ratio) on NHWC bf16|f32 input
     * group_modules.py:26-30 (modules.py:59-60)
     * p0=x [B,H,W,ldx] (bf16, or f32 if flags&1) p1=y bf16 [B,H/r,W/r,ldy] (channels [0,C); channels
     * [C,Cz) are zero-filled)   i: 0 B 1 H 2 W 3 C 4 ldx 5 ldy 6 r 7 Cz */
    CUTIE_OP_AREA_DOWN = 5,
    /* MASK_DOWN: planar f32 masks [K,H,W] -> 16x area mean -> bf16 [K,h,w,8] = (mask, others, 0..)
     * plus plain f32 copy [K,h,w] of the down-sampled mask (object summarizer).
     * cutie.py:149-150,49-59; object_summarizer.py:62
     * p0=masks f32 [K,H,W] p1=y bf16 [K,h,w,8] p2=m16 f32 [K,h,w] (may be 0)  i: 0 K 1 H 2 W 3 r */
    CUTIE_OP_MASK_DOWN = 6,
    /* GAP: per-(b,c) mean over pixels (nn.AdaptiveAvgPool2d(1)), channel_attn.py:31-32
     * p0=x bf16 [B,HW,C] p1=y f32 [B,C] p2=part f32 [B,ceil(HW/64),C] (deterministic 2-stage sum)   i: 0 B 1 HW 2 C
     * flags&1: only the per-chunk partials are produced (ECA_APPLY finishes the reduction in its prologue) */
    CUTIE_OP_GAP = 7,
    /* ECA_APPLY: y = x * sigmoid(conv1d_k5(gap))[c] + r    channel_attn.py:33-37
     * p0=x bf16 [B,HW,C] p1=gap f32 [B,C] (written: the finished means) p2=w f32[5] p3=r bf16 [B,HW,C] p4=y bf16
     * p5=part f32 [B,ceil(HW/64),C] (GAP partials)   i: 0 B 1 HW 2 C
     * p6 (optional, C = 256) = packed weights bf16 [256] of a Cout = 1, 1x1 conv with fused input ReLU applied to y as stored, p7 = its bias f32 [1]
     *      (may be 0), p8 = its output f32 [B,HW]: the mask_pred head of a transformer block (object_transformer.py:151-164) without a launch */
    CUTIE_OP_ECA_APPLY = 8,
    /* GRU: h' = sig(f)*h*(1-sig(u)) + sig(u)*tanh(n), values=[f|u|n] f32   modules.py:35-43
     * p0=values f32 [B,HW,3C] p1=h f32 [B,HW,C] (in/out) p2=h_bf16 bf16 [B,HW,C] (out)  i: 0 n=B*HW 1 C
     * flags&1: one channel per thread (A/B switch; default: four, 16-byte accesses, when C % 4 == 0 and the buffers are aligned -- same bits) */
    CUTIE_OP_GRU = 9,
    /* SEG_AGG: prob=sigmoid(logit); aggregate -> (K+1) logits at 1/4 res   cutie.py:193-198,
     * tensor_utils.py:47-55      p0=logits f32 [K,h,w] p1=agg f32 [K+1,h,w]   i: 0 K 1 h*w */
    CUTIE_OP_SEG_AGG = 10,
    /* UP4_SOFTMAX: bilinear x4 (align_corners=False) of the K+1 logit planes, softmax over planes
     * cutie.py:199-200   p0=agg f32 [K+1,h,w] p1=prob f32 [K+1,4h,4w] p2=logits_up f32 (may be 0)
     * i: 0 K+1 1 h 2 w
     * flags&1: SEG_AGG fused -- p0 = raw logits f32 [K,h,w], the aggregation runs per tap inside the launch (K+1 <= 16) 
     * flags&2 (with flags&1): the one-pixel-per-thread form (A/B switch; default: four pixels per thread, P <= 8)
     * flags&4 (with flags&1, P <= 8, h, w % 4 == 0): the launch also produces MASK_DOWN(prob[1:], r = 16) for the next frame's pixel fusion:
     *      p3 = m16 f32 [K, H/16 * W/16], p4 = pair bf16 [K, H/16, W/16, i3] (channels 0, 1 written), i3 = channel pitch of pair (8 | 64);
     *      bit-identical to a MASK_DOWN launch on the stored probabilities
     * flags&16 (with flags&4): every lane aggregates its own six source pixels (A/B switch; default: the 6 x 6 source pixels under a 16 x 16
     *      output cell are aggregated once per wave and shared through LDS -- half the VALU instructions, same bits)
     * flags&8 (with flags&1): the kernels with a run-time object count (A/B switch; default: one instantiation per K = 1..7, whose loads are
     *      all in flight together -- same bits)
     * ABI 4: i4 > 1 = clips per launch (grid.y; the four-pixel forms only): clip c reads logits p0 + c*K*h*w and writes prob / logits_up
     *      + c*(K+1)*16hw, m16 + c*K*(hw/16), pair + c*K*(hw/16)*i3 -- per clip exactly the one-clip launch
     * Mixed form (with flags&1, without flags&2 / flags&8): i5 != 0 = the object counts of the i4 clips (3-bit fields); i0 = the largest count + 1.
     *      Clip c (grid.y, block-uniform) reads its K_c logit planes at p0 + start_c * h*w and writes its K_c + 1 planes at prob / logits_up
     *      + (start_c + c) * 16hw, m16 + start_c * (hw/16), pair + start_c * (hw/16) * i3; every block branches ONCE into the code instantiated
     *      for K_c objects, so a clip runs the instructions of its one-clip launch */
    CUTIE_OP_UP4_SOFTMAX = 11,
    /* MASK_MERGE: build the per-object mask planes of a frame with an input mask
     * inference_core.py:259-300.  plane t: src[t] >= 0 -> (idx==src[t]) [idx mode] / fmask[src[t]] [float
     * mode]; else (pred==0 ? 0 : (covered ? 0 : pred[t+1])).  Input mask is un-padded; planes are padded.
     * p0=idx i32 [h0,w0] | fmask f32 [n,h0,w0] p1=pred f32 [Kold+1,H,W] (may be 0) p2=src i32 [Knew]
     * p3=planes f32 [Knew,H,W]   i: 0 h0 1 w0 2 H 3 W 4 pad_left 5 pad_top 6 Knew 7 Kold 8 nfloat
     * flags&1: float mode */
    CUTIE_OP_MASK_MERGE = 12,
    /* AGG_SOFTMAX: prob = softmax(aggregate(planes))   inference_core.py:299-300
     * p0=planes f32 [K,HW] p1=prob f32 [K+1,HW]   i: 0 K 1 HW */
    CUTIE_OP_AGG_SOFTMAX = 13,
    /* LINEAR: small-M f32 linear for the object-query side (M = K*16 rows)
     * y = act(x @ W^T + b) + res     nn.Linear / MHA in/out projections, transformer_layers.py
     * p0=x f32 [M,ldx] p1=x_add f32 [M|16, Kd] (added to x before the product, may be 0)
     * p2=W bf16 [N,Kd] p3=bias f32 [N] p4=res f32 [M,N] (may be 0) p5=y f32 [M,ldy]
     * i: 0 M 1 N 2 Kd 3 ldx 4 ldy 5 add_rows (x_add row = m % add_rows)
     *    6 add_cols (> 0: x_add feeds only the output columns < add_cols, e.g. merged [q|k|v] projections where
     *      only q and k see the positional term; multiple of 16)
     * flags&1 relu   flags&2 fused nn.LayerNorm on x first (Kd == 256): p6=gamma f32[Kd] p7=beta f32[Kd]
     *      p8=ln_out f32 [M,Kd] (may be 0: the normalised rows, which the reference reuses as residual) f0=eps */
    CUTIE_OP_LINEAR = 14,
    /* LAYERNORM over the last dim (eps 1e-5)   p0=x f32 [M,C] p1=g p2=b f32[C] p3=y f32 [M,C]  i: 0 M 1 C */
    CUTIE_OP_LAYERNORM = 15,
    /* QUERY_INIT: obj_values = sums/(area+1e-4)   object_transformer.py:125-132
     * p0=obj_mem f32 [K,Q,C+1] p1=y f32 [K*Q,C]   i: 0 K*Q 1 C
     * flags&1 (C == 256, Q == 16): with the two linears that consume it (:137-138) -- p1=query p2=query_emb f32 [K*Q,256],
     *      p3/p4/p5 = W bf16 [256,256], bias, residual f32 [K*Q,256] of summary_to_query_init (+ query_init.weight), p6/p7/p8 of ..._emb
     *      side job: p9 (may be 0, 16-byte aligned) = a range of i2 x 16 bytes that is cleared (the accumulators of the chain forms below) */
    CUTIE_OP_QUERY_INIT = 16,
    /* AUX_MASK: foreground mask from mask_pred logits   object_transformer.py:179-205
     * p0=logits f32 [K,HW] p1=fg u8 [K,HW] p2=nfg i32 [K] (must be zeroed: MEMSET op before)
     * i: 0 K 1 HW */
    CUTIE_OP_AUX_MASK = 17,
    /* ATTN_Q2P: masked cross attention, 16 object queries <- HW pixels, 8 heads x 32
     * transformer_layers.py:45-98 (nn.MultiheadAttention core), object_transformer.py:56-61
     * p0=q f32 [K,Q,C] (projected) p1=kv bf16 [K,HW,ldkv] (k at +0, v at +voff) p2=fg u8 [K,HW]
     * p3=nfg i32 [K] p4=y f32 [K,Q,C]   i: 0 K 1 Q 2 HW 3 C 4 heads 5 ldkv 6 voff
     * flags&1: AUX_MASK fused -- p2=mask_pred logits f32 [K,HW] instead of fg, p3 unused (HW <= 24576)
     * flags&2 (with flags&1, C == 256): the q projection runs inside the launch -- p0=x f32 [K*Q, i7] unprojected rows, p3=ln_out f32
     *      [K*Q,256] (LayerNorm'd rows, may be 0), p5=Wq bf16 [C,256] p6=bias f32 [C] p7=query embedding f32 [K*Q,256] (may be 0)
     *      p8/p9=LayerNorm gamma/beta (0: no norm): q = (LN(x) + emb) Wq^T + b   (the LINEAR op it replaces: transformer_layers.py:86-93)
     * Chain form (flags&8, with flags 1|2; csrc/qchain.hip): the output projection runs inside the launch, per head, and is ADDED in
     *      fixed point to p13 = int64 [K*Q, 256] (value x 2^32; integer atomics: the sum is independent of the order of arrival; the
     *      caller clears it beforehand, e.g. QUERY_INIT's side job); p12 = Wo bf16 [256,256]; p4 is not written.  Wo's bias and the
     *      residual are added by the consumer through ITS flags&4:
     * flags&4 (chain form): the rows are a sum, x_eff = p0 + p11 (bias f32 [256], may be 0) + p10 / 2^32 (p10 = int64 [K*Q, 256])
     * i8 (chain form; 0 = 32): elements between the heads' k (and v) slices inside a pixel row -- 64 with i6 = 32 reads k | v interleaved per
     *      head (one 128-byte line per pixel and head)
     * flags&16 (chain form, instead of flags&4 and of the projection operands): p0 = q f32 [K*Q, 256], already projected and scaled by
     *      1/sqrt(32) (ATTN_P2Q flags&16 of the previous transformer block produces it); p3, p5..p11 unused
     * ABI 4 (chain form): i9 > 0 = objects per clip (clips in lock step): the foreground mask of object k is decided among the i9 objects
     *      of its own clip (logit planes (k / i9) * i9 ...), as object_transformer.py:179-205 aggregates over one video's objects
     * Mixed form (chain form): i10 != 0 = the clips' object counts (3-bit fields, sum = K; i9 = 0): object k's mask is decided among the
     *      K_c objects of its clip (logit planes start_c ..) */
    CUTIE_OP_ATTN_Q2P = 18,
    /* ATTN_SELF: 16x16 self attention per object  transformer_layers.py:12-41
     * p0=qk f32 [K,Q,ldqk] (q at +0, k at +C) p1=v f32 [K,Q,ldv] p2=y f32 [K,Q,C]
     * i: 0 K 1 Q 2 C 3 heads 4 ldqk (0: 2C) 5 ldv (0: C)
     * flags&2 (C == 256): the packed q|k|v in-projection runs inside the launch -- p0=x f32 [K*Q, i6], p3=ln_out (may be 0),
     *      p5=Wqkv bf16 [3C,256] p6=bias f32 [3C] p7=query embedding (q and k only) p8/p9=LayerNorm gamma/beta; p1 unused
     * flags&8 (+ optional flags&4): chain form as ATTN_Q2P (p10, p11 = accumulator input; p12, p13 = output projection into an accumulator;
     *      p2 is not written) */
    CUTIE_OP_ATTN_SELF = 19,
    /* ATTN_P2Q: pixels <- 16 queries cross attention  object_transformer.py:66-70
     * p0=q bf16 [K,HW,ldq] p1=kq f32 [K,Q,ldkv] p2=vq f32 [K,Q,ldkv] p3=y bf16 [K,HW,C]
     * i: 0 K 1 Q 2 HW 3 C 4 heads 5 ldq 6 ldkv (0: C)
     * flags&2 (C == 256): the packed k|v projection of the object queries runs inside the launch -- p1=x f32 [K*Q, i7],
     *      p5=Wkv bf16 [2C,256] p6=bias f32 [2C] p7=query embedding (k only); p2 unused
     * flags&4: chain form, accumulator input as ATTN_Q2P (p10, p11)
     * flags&16 (chain form): extra blocks also project the NEXT transformer block's ATTN_Q2P queries from the same rows x_eff:
     *      p15 = xn_out f32 [K*Q,256] = LN(x_eff; p8 gamma, p9 beta), p14 = q_out f32 [K*Q,256] = ((xn_out + p7) p12^T + p13) / sqrt(32)
     *      (p12 = Wq bf16 [256,256], p13 = bias) */
    CUTIE_OP_ATTN_P2Q = 20,
    /* SUMMARIZE: weights=sigmoid(logits)*[m x8 | (1-m) x8]; sums=einsum; area   object_summarizer.py:11-23
     * p0=feature bf16 [K,HW,C] p1=wlogits f32 [K,HW,Q] p2=m16 f32 [K,HW] p3=y f32 [K,Q,C+1]
     * p4=scratch f32 [K,ceil(HW/128),Q,C+1] (deterministic 2-stage sum)
     * flags&1: p0 is f32 with a row stride of i4 elements (0 = C); i5 = row stride of the logits (0 = Q) -- both read from one conv output
     * [feature | logits] (ABI 3)
     * i: 0 K 1 HW 2 C 3 Q 4 ldf 5 ldw */
    CUTIE_OP_SUMMARIZE = 21,
    /* ADD_PE: y = x + pe (broadcast over objects), bf16     object_summarizer.py:74-76
     * p0=x bf16 [B,HW,C] p1=pe bf16 [HW,C] p2=y   i: 0 B 1 HW*C */
    CUTIE_OP_ADD_PE = 22,
    /* KEY_PREP: split-bf16 MFMA operands of the anisotropic-L2 similarity  memory_utils.py:30-42
     * memory side (flags=0): A=[k^2|k] -> A_hi,A_lo bf16 [n,128], scale=shrinkage/sqrt(CK) f32 [n]
     * query side  (flags=1): B=[-e|2*k*e] -> B_hi,B_lo, c=sum(e*k^2)
     * p0=key f32 [n,64] p1=shr f32 [n] (mem) | sel f32 [n,64] (query) p2=hi p3=lo p4=scale|c   i: 0 n
     * flags&2 (query side): c summed by one lane per row in a 64-step loop (A/B switch; default: the row's lanes hand the running sum on --
     *      the same additions in the same order) */
    CUTIE_OP_KEY_PREP = 23,
    /* AFF_SCORE: S = scale_i*(A_i.B_j - c_j) tiles on MFMA (3-term split bf16: within ~7e-5 of the magnitude sum, see affinity.hip)
     * mode 0: per-(16-token tile, query) maxima -> gmax f32 [HWp, Gld] (query-major, Gld = G rounded up to 64)
     * mode 1: append (S,token) with S >= tau_j to cand lists (f32,i32) [HW,cap], count i32 [HW*32] (counter of query j at [32*j]: one 128-B line each)
     * memory_utils.py:7-46 get_similarity + the candidate pre-filter of top-k (:58)
     * p0=A_hi p1=A_lo p2=scale (bank base pointers, rows = physical token slots) p3=B_hi p4=B_lo p5=c
     * p6=gmax | tau f32 [HW]  p7=cand_val p8=cand_idx p9=count
     * i: 0 HW 1 HWp 2 nranges 3.. (start,n) x3  9 G 10 cap 11 mode  12 query column sets (of 16) per wave: 1 | 2 (0 = 2) | 4 (aff_score4_kernel:
     *      256-query blocks, LDS-DMA staging; same bits for every choice)  13 tiles per block (0 = heuristic)  14 (diagnostic) KB of extra dynamic LDS  15 = 1: aff_score4_kernel (LDS-DMA staging) also for 2 sets per wave
     * flags&1 (mode 1): the gmax matrix of the mode-0 pass lies directly in front of tau in memory (p6 - HWp*Gld floats): every
     *      (16-token tile, 16-query set) whose maximum is below the set's thresholds is skipped (same result, ~1/6 of the MFMA work)
     * ABI 3 -- one read-out per bank version (memory_manager.py:112-208 reads once per frame; the bank changes on memory frames only,
     *      inference_core.py:238): i16 > 0 = query rows per frame; i1 (HWp) is then frames x i16 and the query operands of the frames are
     *      stacked (row j is a real query iff j % i16 < i0); c, gmax, tau, the candidate lists and counters are indexed by the stacked row.
     *      Per query the arithmetic is that of the one-frame launch (same bits).
     * ABI 4 -- clips in lock step (no counterpart in the reference: one InferenceCore, hence one bank, per video, eval_vos.py:97): flags&4 = the
     *      stacked frames read DIFFERENT banks, frame e the bank e % i17; p11 = u64 [i17][3] device table of the banks' (A_hi, A_lo, scale) bases
     *      (p0..p2 are ignored), the token ranges i3..i9 are those of every bank (banks on one schedule).  Needs 2 column sets per wave (i12),
     *      i16 % 128 == 0 (a block's 128 query rows lie inside one frame) and frames % i17 == 0; per query the bits of the one-frame launch
     *      on that frame's bank. */
    CUTIE_OP_AFF_SCORE = 24,
    /* AFF_SELECT: tau_j = top_k-th largest of gmax[:,j] (or -inf if G < top_k)
     * p0=gmax f32 [HWp,Gld] p1=tau f32 [HW]   i: 0 HW 1 HWp 2 G 3 top_k
     * optional side jobs (0 = none): p2=count i32 [HW*32]: count[32 q] = 0 for every query (pass 1's candidate counters);
     *      p3=life f32 [i4], p4=life f32 [i5]: += 1 (USAGE_TICK of two token ranges)
     * flags&1: range p3 is CLEARED instead (the usage side buffer of a look-ahead read-out, see USAGE_TICK)
     * flags&2: values per lane in the three sizes 16 | 32 | 64 only (A/B switch; default: ceil(G / 64) rounded up to a multiple of 4)
     * ABI 3: i6 > 1 = that many stacked frames of i1 query rows each (i0 real ones): gmax, tau and the counters are indexed by the stacked row */
    CUTIE_OP_AFF_SELECT = 25,
    /* AFF_READOUT: exact top-k of the candidates (ties -> lower slot), softmax, usage += w,
     * readout[o,j,:] = sum_i w_i V_o[i,:]    memory_utils.py:58-63,75; memory_manager.py:77-88
     * p0=cand_val p1=cand_idx p2=count p3=vptrs u64[K] (device array of per-object value-bank bases,
     * bf16 [slots,CV]) p4=usage f32 [slots] (may be 0) p5=y bf16 [K,HW,CV] p6=overflow i32[1]
     * i: 0 HW 1 cap 2 top_k 3 K 4 CV
     * ABI 3: i5 > 1 = that many stacked frames of i6 query rows each; frame f's read-out goes to y + f * K*HW*CV and its usage to
     *      p4 + f * i7 floats (per-frame side buffers: a look-ahead read-out is counted when -- and only when -- its frame is consumed)
     * ABI 4: i8 > 1 = that many banks, frame f gathers from bank f % i8: p3 = u64 [i8][K] (see AFF_SCORE flags&4)
     * ABI 4: flags&1 = p4 holds unsigned 64-bit FIXED-POINT counters (2^-40; i7 counts them) instead of f32: integer atomics commute, so the usage
     *      sums do not depend on the order in which the blocks arrive (the f32 form's last bits do); USAGE_TICK flags&1 adds them to the fp32 bank
     *      counters with one rounding.  The reference's usage is a dense column sum (memory_utils.py:58-63, kv_memory_store.py:151-162). */
    CUTIE_OP_AFF_READOUT = 26,
    /* MEMSET32: fill n 32-bit words with value i[1]   p0=dst   i: 0 n 1 value */
    CUTIE_OP_MEMSET32 = 27,
    /* COPY2D: rows x rowbytes strided device copy (bank append / compaction; replaces torch.cat,
     * kv_memory_store.py:7-16)   p0=src p1=dst   i: 0 rows 1 rowbytes(mult of 4) 2 src_stride 3 dst_stride
     * Mixed form: i4 != 0 = the object counts of the clips of a lock-step group (3-bit fields, sum = rows): destination row r -- an object --
     *      is a copy of source row clip(r): a per-clip map (x_transform of MainToGroupDistributor, group_modules.py:112-115) expanded to one map
     *      per object.  rowbytes, both strides and both pointers multiples of 16 */
    CUTIE_OP_COPY2D = 28,
    /* AXPY: y[i] += a * x[i] (f32)  streaming object-memory sum, memory_manager.py:264-269
     * p0=x p1=y  i: 0 n  f: 0 a */
    CUTIE_OP_AXPY = 29,
    /* USAGE_TICK: life[i] += 1 for i in [0,n)   kv_memory_store.py:161  p0=life  i: 0 n
     * optional (0 = none): p1=life2 f32 [i1]: += 1;  p2=use f32 [i2], p3=delta f32 [i2]: use += delta (the usage of a
     * look-ahead read-out, accumulated into a side buffer by AFF_READOUT and applied when the read-out is consumed)
     * ABI 4: flags&1 = p3 holds unsigned 64-bit fixed-point sums (2^-40, AFF_READOUT flags&1), converted with one rounding for every 64-bit
     *      value (the correctly rounded fp32 of d / 2^40: u64 -> f32, then an exact power of two); flags&2 = and is
     *      cleared behind the addition (the side counters of a read-out that is always consumed) */
    CUTIE_OP_USAGE_TICK = 30,
    /* RANK_SELECT: order[r] = index of the r-th largest of use/life (ties -> lower index), r < k
     * torch.topk(usage, k) of memory_manager.py:339 and kv_memory_store.py:222
     * p0=use f32[n] p1=life f32[n] p2=order i32[k] p3=scratch i32[16*n] (partial ranks; required since ABI 3)
     * optional side jobs of the scattering launch: p4/p5, p6/p7 = src/dst of up to two row gathers dst[r,:] = src[order[r],:]
     * (rows of i2 / i3 32-bit words, multiples of 4: the prototype keys / selections of memory_manager.py:341-345);
     * p8 = u32 buffer of i4 words cleared (the column maxima of CONSOL_AFF)
     * i: 0 n 1 k 2 row words of gather 1 3 row words of gather 2 4 words to clear
     * refused: n < 1 and k > n (order[n .. k) would keep what an earlier call left there; torch.topk raises) */
    CUTIE_OP_RANK_SELECT = 31,
    /* GATHER_ROWS: dst[r,:] = src[order[r],:]   p0=src p1=order i32 p2=dst  i: 0 k 1 rowbytes 2 src_stride 3 dst_stride */
    CUTIE_OP_GATHER_ROWS = 32,
    /* CONSOL_AFF (ABI 3): similarities of long-term consolidation, memory_manager.py:347-350 / memory_utils.py:30-42
     * S[p,i] = sim(cand_i, proto_p) for i < n, -inf for n <= i < ldS; colmax[p] = max_i S[p,i] as an order-preserving u32 key,
     * accumulated by atomicMax into a buffer the caller cleared (RANK_SELECT p8)
     * p0=ckey f32 [n,64] p1=cshr f32 [n] p2=pkey f32 [P,64] p3=psel f32 [P,64] p4=S f32 [P,ldS] p5=colmax u32 [P]
     * i: 0 n 1 P 2 ldS (multiple of 32, >= n) */
    CUTIE_OP_CONSOL_AFF = 33,
    /* CONSOL_READ (ABI 3): prototypes = softmax_i(S[p,:]) applied to the candidates' values of every object and to their shrinkage
     * memory_manager.py:347-356 (softmax over the candidates with max shift, memory_utils.py:68-71; aff @ values)
     * value rows of object o: candidates at vptrs[o] + (src + i) * C, prototypes written to vptrs[o] + (dst + p) * C (bf16);
     * out_shr[p] = sum_i softmax(S)[p,i] * cshr[i]
     * p0=S f32 [P,ldS] p1=colmax u32 [P] p2=vptrs u64 [K] p3=cshr f32 [n] p4=scratch f32 [nchunk * (K*P*C + 2*P)], nchunk = ceil(ldS/256)
     * p5=out_shr f32 [P] (or 0)
     * i: 0 n 1 P 2 C (multiple of 128) 3 K 4 ldS 5 src slot 6 dst slot */
    CUTIE_OP_CONSOL_READ = 34,
    /* CAST: f32 [n] -> bf16 [n] (flags=0) or bf16 -> f32 (flags=1)   p0=src p1=dst  i: 0 n */
    CUTIE_OP_CAST = 35,
    /* PROB_TO_ID: id = lut[argmax over the P planes] -- InferenceCore.output_prob_to_mask (inference_core.py:337-345) and
     * ResultSaver.process (results_utils.py:93-106: argmax + tmp-id -> object-id remap), fused; first maximum wins.
     * p0=prob f32 (P planes of H x W, plane stride i3 elements, row stride i4: the un-padded view that `step` returns
     * is addressed in place) p1=lut i32[P] p2=out [H,W] u8 (flags&3 == 0) | i32 (1) | i64 (2)
     * i: 0 P 1 H 2 W 3 plane stride 4 row stride
     * ABI 7 -- result egress (ResultSaver egress='device', results_utils.py:85-133 of the reference: F.interpolate of the K+1 planes to the
     *    original size, argmax + remap, .cpu(), PIL's PNG encoder on a writer thread); flags other than 1 | 2 | 4 | 8 are an error:
     *  flags&4: the planes are resampled to i5 x i6 (OH x OW) inside the launch -- bilinear, align_corners=False, no antialias: per plane
     *    exactly RESIZE's (flags == 0) sample, the same source index, lambdas and order of multiplies and adds -- and the argmax is taken
     *    of the samples: out = [OH, OW], u8 | i32 (flags&3 == 2 is an error), bit-identical to RESIZE followed by PROB_TO_ID without the
     *    P x OH x OW floats in memory.  OH == H and OW == W runs the plain kernel.
     *  flags&8: PNG scanline filter + DEFLATE + Adler-32 (kernels in png.hip) of the uint8 id plane p2 ([OH, OW] with flags&4, else [H, W];
     *    flags&3 must be 0), after the id stage or -- p0 == 0 -- on its own on an existing plane (i0, i3, i4 unused).
     *    p3 = stream uint8, 4-byte aligned, i7 = its capacity in bytes (rounded down to a multiple of 4): the complete zlib stream -- 2-byte
     *    header, ONE final DEFLATE block with the fixed Huffman codes, big-endian Adler-32 -- whose inflation is the filtered image, every
     *    row = filter byte 0 + its W ids.  ceil(((W + 1) * H * 9 + 10) / 8) + 6 bytes hold any plane (a literal costs at most 9 bits).
     *    p4 = status int32 [4], written by the launch: 0 stream bytes, 1 Adler-32, 2 error bits (1: the stream does not fit the capacity;
     *    NOTHING is written to p3 then -- with i7 < 4 it may be null --, [0] still says what it needs), 3 zero.  p5 = int32 scratch of i8 words, 16-byte aligned,
     *    i8 >= H * (4 + ceil(9 (W + 1) / 32) + 2).  W <= 32767 (a row is one match distance).  The bytes depend on the plane alone.
     *    cutie_amd/inference/utils/png.py wraps the stream into a file (signature, IHDR, PLTE, one IDAT, IEND).
     * ABI 8 -- multi-scale merge on the device (scripts/merge_multi_scale.py of the reference: the uint8 score dumps of several runs are
     *    summed and the argmax of the sum is the mask; ResultSaver.process_merged, eval_vos --sizes); flags other than 1 | 2 | 4 | 8 | 16 are
     *    an error:
     *  flags&16: the ids of S sources merged.  Per output pixel and plane q: sum[q] = sum over the sources s of (int)(uint8)(sample_s * 255.f)
     *    -- sample_s = exactly the flags&4 (= RESIZE flags == 0) sample of source s at the pixel, quantised by TRUNCATION as
     *    (prob * 255).to(torch.uint8) / numpy astype(uint8) do -- in 32-bit integers, so the result depends neither on the order of the
     *    sources nor on the launch shape; id = lut[first q with the largest sum].  Every source has its own size and strides; one whose size
     *    equals the output samples itself exactly.  flags&4 MUST accompany flags&16 (the output geometry is that path's i5 x i6; 16 alone is
     *    an error); flags&3 is 0 | 1 (u8 | i32; 2 is an error); combines with flags&8 (unchanged).  Slots that differ from the above:
     *    p0 = u64 [S] device table: the sources' first planes (f32, P planes each, last dimension contiguous), 8-byte aligned
     *    p6 = i32 [S, 4] device table, 16-byte aligned: per source H, W, plane stride, row stride (elements; H, W >= 1 -- a source that says
     *    otherwise is left out of the sum)       i9 = S, 1 <= S <= CUTIE_MERGE_MAX_SOURCES       i1 .. i4 unused.
     *    The launcher checks what it can see (flags, S, null / misaligned tables, P, OH, OW); the tables' contents are the caller's.
     * ABI 9 -- BURST egress (results_utils.py:153-171 of the reference: per annotated frame and object, pycocotools' mask_util.encode of
     *    (mask == id), its counts string into predictions.json; ResultSaver egress='device' with init_json):
     *  flags == 32, a stage ON ITS OWN (32 combined with any other flag stays the "unknown flags" error): the COCO compressed-RLE strings of
     *    the objects of an existing uint8 id plane p2 = [i1, i2] = [H, W], row-major and contiguous (kernels in rle.hip; the format and
     *    its numpy model: cutie_amd/inference/utils/coco_rle.py -- the mask flattened column-major, run lengths from a run of zeros on,
     *    count j > 2 as counts[j] - counts[j-2], 5-bit groups + 48).  i0, i3 .. i6 and p0, p1 unused.
     *    p6 = object ids int32 [i9], 4-byte aligned, i9 = n <= 255: distinct ids 1 .. 255; ids of the plane that are not listed are
     *    background for every listed object; an entry 0, above 255 or equal to an earlier entry is encoded as an absent object.
     *    p3 = stream uint8 (any alignment), i7 = its capacity in bytes: the n strings back to back in the order of p6, no separators.
     *    p7 = table int32 [n, 4], 16-byte aligned: per object byte offset, bytes, number of counts, area (an absent object: one count
     *    H * W, area 0).  p4 = status int32 [4], 4-byte aligned: 0 bytes of all strings (saturating at 2^31 - 1), 1 error bits (1: the
     *    strings do not fit the capacity; NOTHING is written to p3 then and the table's offsets are 0; bytes, counts and areas stay valid),
     *    2 counts of all strings, 3 zero.  With n == 0 only the status is written (p6, p7 may be null).
     *    p5 = int32 scratch of i8 words, 16-byte aligned, i8 >= 1024 + roundup4(ceil(G / 1024)) + n * W * ceil(H / 256) + G with
     *    G = 2 H W + n (cutie_amd/ops.py OpList.rle_scratch_words): per-object sums, one word per 1024 run boundaries, the run starts
     *    per (object, chunk of <= 256 rows of one column), and the boundary positions -- at most two per pixel, one sentinel per object.
     *    H * W < 2^31.  One sweep over the plane finds the runs of all objects (the transposition happens in LDS tiles); every offset
     *    comes from a scan in a fixed order, the per-object byte and area totals from integer atomics: the bytes depend on the plane and
     *    the object list alone, not on launch shape or timing.  The launcher refuses, each with its own message and before any launch:
     *    H, W < 1, H * W >= 2^31, n outside 0 .. 255, a negative capacity, a null or misaligned pointer, a scratch that is too small.
     * ABI 10 -- DAVIS J&F on the device (not in the reference, whose docs/EVALUATION.md hands the PNG folder to davis2017-evaluation; here
     *    eval_vos --score, cutie_amd/inference/utils/davis_metrics.py; the arithmetic is that package's metrics.py / utils.py seg2bmap):
     *  flags == 64, a stage ON ITS OWN (64 combined with any other flag stays the "unknown flags" error): the integers of J and F of a
     *    predicted id plane p2 against a ground-truth id plane p3, both uint8 [i1, i2] = [H, W], row-major and contiguous (kernels in
     *    score.hip; the numpy / scipy model: tests/jf_ref.py).  i0, i3, i4, i6, i7 and p0, p1, p4 unused.
     *    p6 = object ids int32 [i9], 4-byte aligned, i9 = n, 1 <= n <= 255: every entry is scored on its own as the binary masks
     *    P = (p2 == id) and G = (p3 == id); values of the planes that are not listed are background for every listed object, in both
     *    planes -- so ground-truth 255 (DAVIS void) never matches, as after davis2017's get_all_masks has zeroed it (the package also
     *    takes the void pixels out of the prediction; this stage does not: a known difference).  Entries are 1 .. 254; any other
     *    entry is scored as an absent object (all counts 0); an entry equal to an earlier one gets the same counts again.
     *    i5 = r, the match radius, 1 <= r <= CUTIE_JF_MAX_RADIUS; the host computes ceil(0.008 * sqrt(H*H + W*W)) in float64.
     *    p7 = counts int32 [n, 8], 16-byte aligned, WRITTEN by the launch (whatever it held before): per object 0 |P & G|, 1 |P | G|,
     *    2 boundary pixels of P, 3 boundary pixels of G, 4 boundary pixels of P within r of a boundary pixel of G, 5 boundary pixels of G
     *    within r of a boundary pixel of P, 6 |P|, 7 |G|.  Boundary map = seg2bmap at equal size: b = (s ^ e) | (s ^ so) | (s ^ se) over the
     *    east, south and south-east neighbours; the last row uses s ^ e only, the last column s ^ so only, the bottom-right pixel is 0.
     *    "Within r": B has a boundary pixel at (y + dy, x + dx) inside the image with dy*dy + dx*dx <= r*r -- dilation by disk(r) with
     *    nothing outside the image.
     *    p5 = int32 scratch of i8 words, 16-byte aligned, i8 >= 4 * n * H * ceil(W / 64) (cutie_amd/ops.py OpList.jf_scratch_words): the
     *    boundary bit planes of both ids planes per object, one 64-bit word per 64 columns of a row.
     *    H * W < 2^31, so every count fits.  All sums are integers gathered with integer atomics: the counts depend on the planes, the
     *    object list and r alone, not on launch shape or timing.  The launcher refuses, each with its own message and before any launch:
     *    H, W < 1, H * W >= 2^31, n outside 1 .. 255, r outside 1 .. 40, a null or misaligned pointer, a scratch that is too small.
     * ABI 11 -- the --visualize overlays on the device (results_utils.py:173-192 of the reference: per frame the image is decoded again, the
     *    object colours are blended over it in float and PIL writes <frame>.jpg; ResultSaver overlay='device', eval_vos --overlay device):
     *  flags == 128, a stage ON ITS OWN (128 combined with any other flag stays the "unknown flags" error): the entropy-coded segment of
     *    the baseline JPEG (4:2:0, standard Huffman tables, no restart markers) of a frame with the colours of an id plane blended over
     *    it -- the bytes libjpeg-turbo's encoder (PIL's Image.save) writes for the blended frame (kernels in jpeg_enc.hip; the numpy model:
     *    tests/jpeg_enc_ref.py; header and EOI: cutie_amd/inference/utils/jpeg_writer.py).  i0, i3, i5, i6 and p1 unused.
     *    p0 = frame uint8 [i1, i2, 3] = [H, W, 3], pixels packed, row stride i4 BYTES (>= 3 W), any alignment.
     *    p2 = id plane uint8 [H, W], row-major and contiguous, or 0: the frame is encoded as it is (p6 unused then).
     *    p6 = colour table uint8 [256][4] (R, G, B, unused), 4-byte aligned: one colour per id; entry 0 is never read; an id that is
     *    not an object gets the colour 0 and is still halved, as on the host.
     *    p7 = quantisation tables uint16 [2][64] (luminance, chrominance), NATURAL (row-major) order, 2-byte aligned, values 1 .. 255.
     *    p3 = stream uint8 (any alignment), i7 = its capacity in bytes: the segment, byte-stuffed and padded to a byte with 1-bits.
     *    p4 = status int32 [4], 4-byte aligned, written by the launch: 0 stream bytes (saturating at 2^31 - 1), 1 zero, 2 error bits (1:
     *    the stream does not fit the capacity; NOTHING is written to p3 then -- with i7 == 0 it may be null --, [0] still says what it
     *    needs), 3 zero: the PNG stage's convention.
     *    p5 = int32 scratch of i8 words, 16-byte aligned, i8 >= 16 + 36 B + (52 B + 16) + 4 ceil((52 B + 16) / 16) with B = 6 ceil(W / 16)
     *    ceil(H / 16) coded blocks (cutie_amd/ops.py OpList.jpeg_enc_scratch_words): a header, per block 64 int16 coefficients, a 64-bit
     *    bit offset and a bit count, the unstuffed stream at the worst case of 1660 bits per block (22 of DC, 63 x 26 of AC), and per
     *    64-byte chunk of it the 0xFF count and its scan.  2 ceil(1660 B / 8) bytes hold any stream (OpList.jpeg_enc_capacity).
     *    The rules (libjpeg-turbo's encoder path, each checked against PIL by tests/test_jpeg_encode_cpu.py through the model):
     *    - blend: id == 0: the frame's pixel; else (frame + colour[id]) >> 1 per channel (= the host's float blend, truncated).
     *    - colour (SCALEBITS 16): Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
     *      Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16.
     *    - geometry: Y has ceil(W / 8) x ceil(H / 8) blocks, Cb and Cr ceil(ceil(W / 2) / 8) x ceil(ceil(H / 2) / 8); ceil(W / 16) x
     *      ceil(H / 16) MCUs, coded row by row, each Y00 Y01 Y10 Y11 Cb Cr.
     *    - edges: Y replicates its last column and row out to whole blocks.  Chroma replicates the INPUT's last column as far as needed and
     *      its last row once if H is odd, averages 2 x 2 as (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2, ... along the output
     *      columns, and then replicates the last DOWNSAMPLED row out to whole blocks.
     *    - dummy blocks: a Y block of an MCU beyond the component's block grid (ceil(W / 8) or ceil(H / 8) odd) has all AC zero and the DC
     *      of the block coded just before it: DC difference 0 + EOB, and the DC prediction passes over it.
     *    - FDCT: jfdctint (ISLOW) on sample - 128: CONST_BITS 13, PASS1_BITS 2, rows then columns, DESCALE with rounding.  32-BIT
     *      INTERMEDIATES SUFFICE: pass-1 outputs are <= 4096 in magnitude, so no pass-2 sum of products exceeds 1.13e9 (the bound is
     *      worked out in jpeg_enc.hip; the model computes in 64 bits and asserts the 32-bit range on everything it encodes).
     *    - quantisation: divisor d = q << 3, sign(c) * ((|c| + (d >> 1)) / d).
     *    - coding: tables K.3 - K.6; DC = the difference to the component's previous block in coded order (0 at the start); AC with ZRL
     *      for runs above 15 and EOB unless the last coefficient is nonzero; bits MSB first, every 0xFF byte followed by 0x00, the last
     *      byte filled with 1-bits (and stuffed like any other).
     *    Every offset comes from a scan in a fixed order and bits shared by two blocks are merged with an integer OR: the bytes depend on
     *    the inputs alone, not on launch shape or timing.  The launcher refuses, each with its own message and before any launch: H, W < 1,
     *    H, W > 65535, H * W >= 2^31, a negative capacity, a null pointer (p0, p3 with i7 > 0, p4, p5, p7, p6 with p2), a misaligned
     *    pointer (p4, p5, p6, p7), a frame row stride < 3 W, a scratch that is too small.
     * ABI 11, forms added (the version number stays 11: both flag values were the "unknown flags" error before, so a library without them
     *    refuses such a descriptor by message instead of misreading it, and no existing descriptor changes meaning) -- the visualisation modes, the alpha matte and the soft masks of the reference's interactive tool on the device
     *    (gui/interactive_utils.py:79-229 get_visualization_torch, gui/resource_manager.py:154-173; ResultSaver vis_modes / soft_masks /
     *    alpha_matte, process_video --vis / --soft-masks / --alpha; kernels in matte.hip; the numpy model: tests/matte_ref.py; the
     *    reference's bytes: tests/golden/matte/).  Two stages, each ON ITS OWN (256 or 512 combined with any other flag stays the
     *    "unknown flags" error).  The arithmetic of both: float32, every multiply and add rounded on its own (no contraction).
     *    im[c] = (float)frame[c] / 255.0f, correctly rounded (RESIZE flags&4).  p_q = plane q at the output pixel: the plane itself when
     *    (H, W) == (OH, OW), else exactly the flags&4 (= RESIZE flags == 0) sample -- the same source index, lambdas and order of operations.
     *    m = the sum of p_q over the target planes, added in list order starting from the first; 0 for an empty list.
     *    Every output byte is (uint8)(x * 255.0f) with the product clamped to [0, 255] (NaN: 0) -- truncation, torch's .byte().
     *  flags == 256, composite: ONE mode of one frame.
     *    i0 = P, i1 = H, i2 = W, i3 = plane stride, i4 = row stride (elements) of p0 = planes f32, 4-byte aligned (the un-padded view
     *    that `step` returns is read in place); soft modes only -- the hard modes ignore them.  i5 = OH, i6 = OW: the output size.
     *    i8 = mode: 0 davis, 1 light, 2 fade (hard modes), 3 popup, 4 layer (soft modes), 5 alpha (the matte plane alone).
     *    p2 = frame uint8 [OH, OW, 3], pixels packed, row stride i7 BYTES (>= 3 OW), any alignment (modes 0 .. 4).
     *    p3 = out uint8 [OH, OW, 3], packed and contiguous, 16-byte aligned (modes 0 .. 4).
     *    p1 = target list int32 [i9] in HOST memory, 4-byte aligned, i9 <= 255 plane indices 0 .. P - 1 (soft modes): the launcher reads
     *    and checks it during the call and hands the kernel a copy, so it may change or go away afterwards.
     *    p4 = matte uint8 [OH, OW], contiguous, 16-byte aligned: clamp(m, 0, 1) quantised -- the fourth channel of the reference's
     *    'rgba' mode.  Optional with popup and layer (the launch then writes both), required with alpha, an error with a hard mode.
     *    Hard modes: p5 = id plane uint8 [OH, OW], contiguous, 4-byte aligned; p6 = colour table uint8 [256][4] (R, G, B, unused), 4-byte
     *    aligned.  col = table[id] / 255.0f;  id != 0: x = im * a + b * col with a = (float)alpha, b = (float)(1.0 - alpha) (the
     *    subtraction in double), alpha = 0.5 (davis, fade) | 0.9 (light);  id == 0: x = im, for fade x = im * 0.6f.  An id that is not
     *    an object blends whatever the table holds for it.
     *    popup: g = (im[0] * 0.3f + im[1] * 0.59f) + im[2] * 0.11f;  x = m * im + (1.0f - m) * g.
     *    layer: p7 = layer uint8 [OH, OW, 4] RGBA, contiguous, 16-byte aligned; la = L[3] / 255.0f, lr = L[0..2] / 255.0f;
     *    x = clamp((im * ((1 - m) * (1 - la)) + (lr * (1 - m)) * la) + im * m, 0, 1).
     *  flags == 512, soft masks: p0, i0 .. i6 as above; p2 = out uint8 [P - 1, OH, OW], contiguous, 16-byte aligned: plane q - 1 =
     *    (uint8)(p_q * 255.0f) for q = 1 .. P - 1 -- the truncation of the merge (flags&16).  P == 1 writes nothing (p2 may be null).
     *  Both are streaming passes without atomics or order-dependent sums: the bytes depend on the inputs alone, not on the launch shape.
     *  The launcher refuses, each with its own message and before any launch: OH, OW < 1 (and H, W < 1 where planes are read),
     *    H * W, 3 * OH * OW or P * OH * OW >= 2^31, P outside 1 .. 256, more than 255 targets or one outside 0 .. P - 1, an unknown
     *    mode, a null or misaligned pointer, a row stride below the row (planes: W elements, frame: 3 OW bytes), the id plane and
     *    colour table missing for a hard mode, the layer for mode layer, the matte plane for mode alpha -- or given with a hard mode.
     * ABI 11, form added (the number stays 11; cutie_hip_build_flags() bit 4, value 16, says the form is present -- a library from before
     *    refuses such a descriptor as "unknown flags") -- the per-object track report (not in the reference; ResultSaver tracks=...,
     *    eval_vos / process_video --tracks, cutie_amd/inference/utils/track_report.py):
     *  flags == 1024, a stage ON ITS OWN (1024 combined with any other flag stays the "unknown flags" error): per listed object the area,
     *    the bounding box and the coordinate sums of an existing uint8 id plane p2 = [i1, i2] = [H, W], row-major and contiguous, any
     *    alignment -- the plane the PNG is written from -- and, optionally, how sure the model was of the object (kernels in tracks.hip;
     *    the numpy model: tests/track_ref.py).  i7, i8 and p3 .. p5 unused.
     *    p6 = object ids int32 [i9], 4-byte aligned, i9 = n, 0 <= n <= 255.  Ids of the plane that are not listed are background for
     *    every listed object; an entry outside 1 .. 255 is an absent object; an entry equal to an earlier one gets the earlier one's row
     *    again (the flags == 64 convention).
     *    Confidence source, optional: p0 = probability planes f32, 4-byte aligned, or 0.  i0 = P planes of i5 x i6 (h x w) samples, i3 =
     *    plane stride, i4 = row stride (elements, i4 >= w; the un-padded view that `step` returns is addressed in place); p1 = lut int32
     *    [P], 4-byte aligned, plane -> object id, exactly PROB_TO_ID's lut.  With p0 == 0, i0, i3 .. i6 and p1 are unused.
     *    p7 = table int32 [n, 12], 16-byte aligned, WRITTEN by the launch (whatever it held before).  Per object: 0 area, 1 xmin, 2 ymin,
     *    3 xmax, 4 ymax, (5, 6) sum of x, (7, 8) sum of y, 9 confidence sample count, (10, 11) confidence sum; a pair is a 64-bit value,
     *    low word first.  x = column, y = row of the id plane, 0-based.  An object without a pixel (and an absent one): area 0, xmin = W,
     *    ymin = H, xmax = ymax = -1 -- the identities of min and max -- and all sums 0.
     *    Confidence: for every sample of the planes q* = the first plane with the largest value -- prob_to_id_kernel's loop: plane 0,
     *    then every plane whose value is > the best so far, so a NaN never displaces anything and nothing displaces a NaN in plane 0.
     *    If lut[q*] is a listed object, its count grows by 1 and its sum by q16(prob[q*]), q16(v) = 0 if !(v > 0), 65535 if v >= 1, else
     *    (int)(v * 65535.f + 0.5f) (float32, multiply and add rounded on their own): a NaN counts as 0.  With p0 == 0 words 9 .. 11 are 0.
     *    The confidence is taken at the model's resolution -- the numbers the model produced, before any resample to the output size;
     *    box, area and sums come from the id plane at the output size -- they describe the file that is written.
     *    Every sum is an integer sum and every min / max an integer min / max, gathered with integer atomics (registers, then LDS, then
     *    one set of global atomics per block and object; the coordinate and confidence sums in 64 bits all the way: sum of x reaches
     *    H W (W - 1) / 2, beyond 2^32 from 513 x 4096 on): the table depends on the planes, the lists and the lut alone, not on launch
     *    shape or timing.  The launcher refuses, each with its own message and before any launch: H, W < 1, H * W >= 2^31, n outside
     *    0 .. 255, with p0: P outside 1 .. 256, h, w < 1, h * w >= 2^31, a row stride below w; a null or misaligned pointer.  With n == 0
     *    nothing is written (p6, p7 may be null).
     * ABI 11, form added (the number stays 11; cutie_hip_build_flags() bit 5, value 32, says the form is present -- a library from before
     *    refuses such a descriptor as "unknown flags") -- the region filter (not in the reference; ResultSaver min_region= / fill_holes=,
     *    eval_vos / process_video --min-region / --fill-holes):
     *  flags == 2048, a stage ON ITS OWN (2048 combined with any other flag stays the "unknown flags" error): connected components of an
     *    existing uint8 id plane p2 = [i1, i2] = [H, W], row-major and contiguous, any alignment, REWRITTEN IN PLACE: small object
     *    components are dropped and small enclosed background components are filled (kernels in regions.hip; the numpy model:
     *    tests/region_ref.py).  i0, i6, i7, p0, p1, p3, p4, p6 and the floats are unused.
     *    i3 = min_region >= 0, i4 = fill_holes >= 0, i5 = connectivity, 4 (edge neighbours) or 8 (edge and corner neighbours); both
     *    stages use the same one.
     *    p5 = scratch int32, 4-byte aligned, of i8 + 2^31 * i9 words (i8, i9 >= 0): at least 2 * H * W (OpList.region_scratch_words).
     *    Its content before and after the launch means nothing.
     *    p7 = counts int32 [4], 4-byte aligned, WRITTEN by the launch (whatever it held before): 0 islands removed | 1 pixels cleared |
     *    2 holes filled | 3 pixels filled.
     *    Stage A, islands (runs when min_region >= 2): a component is a maximal set of pixels of one non-zero id, connected under i5.
     *    Every id 1 .. 255 is an object, whether or not anyone lists it.  A component of fewer than min_region pixels becomes 0.  All
     *    decisions are taken on the plane as it entered the stage.
     *    Stage B, holes (runs when fill_holes >= 2, on A's result): a component is a maximal set of pixels of id 0, connected under
     *    i5.  A component with a pixel in row 0, row H - 1, column 0 or column W - 1 is never a hole.  Every other component of fewer
     *    than fill_holes pixels is filled with the id of the pixel left of its first pixel in raster order, (y0, x0 - 1) -- which
     *    exists (x0 > 0: the component does not touch column 0) and is not 0 (it would belong to the component and precede (y0, x0)).
     *    Thresholds 0 and 1 switch a stage off (no component has fewer than 1 pixel).  With both below 2 the launch zeroes counts and
     *    does nothing else.
     *    Islands run BEFORE holes, so that a speck of object B inside object A ends up as A: A's stage clears it to a hole, B's stage
     *    fills the hole with A.  (Segment Anything's remove_small_regions, for binary masks, is called holes first, then islands; for
     *    an id plane that order would leave the speck as background inside A, or keep it.)
     *    Determinism: components are linked by atomicMin on linear pixel indices, so a component's root is its smallest linear index
     *    whatever the arrival order -- which also makes the fill pixel root - 1; areas and counts are integer sums.  The plane and
     *    counts after the launch depend on the plane before it and on i3 .. i5 alone.
     *    The launcher refuses, each with its own message and before any launch: H, W < 1, H * W >= 2^31, a negative threshold, a
     *    connectivity other than 4 or 8, a null p2, p5 or p7, p5 or p7 not 4-byte aligned, fewer scratch words than 2 * H * W.
     * ABI 11, form added (the number stays 11; cutie_hip_build_flags() bit 6, value 64, says the form is present -- a library from before
     *    refuses such a descriptor as "unknown flags") -- the exact squared Euclidean distance transform and its bands (not in the
     *    reference; ResultSaver trimap= / trimap_objects= / dilate_mask=, eval_vos / process_video --trimap / --trimap-objects /
     *    --dilate-mask):
     *  flags == 4096, a stage ON ITS OWN (4096 combined with any other flag stays the "unknown flags" error): for each of S sets of ids,
     *    how far every pixel of an existing uint8 id plane p2 = [i1, i2] = [H, W] (row-major and contiguous, any alignment, READ ONLY)
     *    is from the set's edge (kernels in edt.hip; the numpy model: tests/edt_ref.py).  i0, p0, p1, p4 and the floats are unused.
     *    p6 = sets uint8 [S][256], i9 = S, 1 <= S <= CUTIE_EDT_MAX_SETS: id v belongs to set s iff sets[s][v] != 0; an id may be in
     *    several sets or in none.  F_s = the pixels whose id is in set s.
     *    i3 = inner >= 0, i4 = outer >= 0, i5 = limit with max(inner, outer) < limit <= CUTIE_EDT_MAX_LIMIT, i6 = mid, a byte.
     *    Per set: d2(p) = the smallest dx^2 + dy^2, an integer, from p to a pixel of the OTHER class inside the frame -- a pixel of F
     *    looks for one outside F and the reverse.  NOTHING EXISTS OUTSIDE THE FRAME: an object cut by the frame's border is not
     *    eroded from there (the object goes on beyond the picture; scipy's binary_erosion border_value=1).  D(p) = min(d2(p), limit),
     *    and D = limit everywhere when the frame holds no pixel of the other class.  D >= 1.
     *    p7 = dist2 int32 [S, H, W], 4-byte aligned, or null: D(p); any value below limit is the exact d2.
     *    p3 = band uint8 [S, H, W], any alignment, or null: for p in F 255 if D > inner, else mid; for p outside F mid if D <= outer,
     *    else 0.  (Trimap: mid = 128, inner = floor(r_in^2), outer = floor(r_out^2); dilation by the disk dx^2 + dy^2 <= r^2: inner =
     *    0, mid = 255, outer = floor(r^2); erosion: outer = 0, mid = 0.  inner = 0 erodes nothing, outer = 0 dilates nothing.)
     *    Not both null.
     *    p5 = scratch int32, 4-byte aligned, of i8 + 2^31 * i7 words (i7, i8 >= 0): at least ceil(S * H * W / 2)
     *    (OpList.edt_scratch_words).  Its content before and after the launch means nothing.
     *    Determinism: integers only, no atomics, every word written once by one thread and read behind a kernel boundary: the outputs
     *    depend on the plane, the sets and i3 .. i6 alone.
     *    The launcher refuses, each with its own message and before any launch: H, W < 1, H * W >= 2^31, S outside 1 ..
     *    CUTIE_EDT_MAX_SETS, a negative inner or outer, a limit outside max(inner, outer) + 1 .. CUTIE_EDT_MAX_LIMIT, mid outside 0 ..
     *    255, a null p2, p6 or p5, p3 and p7 both null, p5 or p7 not 4-byte aligned, fewer scratch words than needed.
     * ABI 11, form added (the number stays 11; cutie_hip_build_flags() bit 7, value 128, says the form is present -- a library from before
     *    refuses such a descriptor as "unknown flags") -- the outlines of the objects of an id plane as exact polygons (not in the
     *    reference; ResultSaver polygons=, eval_vos / process_video --polygons):
     *  flags == 8192, a stage ON ITS OWN (8192 combined with any other flag stays the "unknown flags" error): every listed object of an
     *    existing uint8 id plane p2 = [i1, i2] = [H, W] (row-major and contiguous, any alignment, READ ONLY) is traced into RINGS of
     *    lattice corners (kernels in polygons.hip; the model: tests/polygon_ref.py).  i0, p0, p1 and the floats are unused.
     *    SET AND LATTICE.  For a listed object with id v, F = {(x, y): plane[y][x] == v}.  Pixel (x, y) is the unit square [x, x + 1] x
     *    [y, y + 1]; lattice vertices are the pixel corners (x, y), 0 <= x <= W, 0 <= y <= H.  Everything outside the frame is "not F":
     *    an object cut by the border is closed along the border (unlike flags == 4096, where nothing exists outside: a polygon closes).
     *    DIRECTED BOUNDARY EDGES.  A boundary edge is a unit edge between a pixel of F and one that is not, directed so that F lies on the
     *    RIGHT of the direction of travel (x right, y down).  For a pixel of F at (x, y), where the neighbour across is not F:
     *      top    E, d = 0: (x, y) -> (x + 1, y)            right  S, d = 1: (x + 1, y) -> (x + 1, y + 1)
     *      bottom W, d = 2: (x + 1, y + 1) -> (x, y + 1)    left   N, d = 3: (x, y + 1) -> (x, y)
     *    An edge is named by its tail vertex and direction: e = (y (W + 1) + x) * 4 + d.
     *    SUCCESSOR.  The next edge starts at the head vertex: the first existing edge of the object there in the order left, straight,
     *    right for connectivity 8 and right, straight, left for connectivity 4.  The two differ only at a SADDLE (the two pixels of one
     *    diagonal in F, the other two not): 8 turns left and crosses to the diagonal pixel -- an 8-connected component is one ring that
     *    touches itself at the vertex --, 4 turns right and stays on its pixel.  The successor is a permutation of the object's boundary
     *    edges; its cycles are the rings.
     *    RING.  A ring's first edge is its edge of smallest e (the smallest (y, x, d) of its tails).  Its vertices are the tails of the
     *    edges whose predecessor has another direction (the corners; collinear lattice points are dropped), in the order of travel from
     *    the first edge's tail, which is a corner.  Consecutive vertices differ in one coordinate, horizontal and vertical steps
     *    alternate, a ring has an even number >= 4 of vertices.  The shoelace sum 1/2 sum(x_i y_{i+1} - x_{i+1} y_i) is positive for an
     *    outer ring and negative for a hole; a ring is a hole iff its first edge is vertical (d = 1; an outer ring's has d = 0); the
     *    signed areas of an object's rings add up to its pixel count.  The rings of an object are ordered by first edge, the objects as
     *    listed.
     *    p6 = object ids int32 [i9], 0 <= n <= 255.  Ids of the plane that are not listed belong to no object; an entry outside 1 .. 255
     *    or equal to an earlier entry is an absent object without rings (the convention of flags == 32).
     *    i5 = connectivity, 4 or 8.  i6 = path: 0 lets the launcher's chain choose (up to 4096 boundary edges are traced by one workgroup
     *    in LDS), 1 forces the general chain; the results are the same words.  i3 = edge capacity E_cap >= 1.
     *    p5 = scratch int32, 16-byte aligned, of i8 + 2^31 * i7 words (i7, i8 >= 0): at least OpList.polygon_scratch_words(H, W, n,
     *    E_cap) = 64 + up4(ceil(NV / 1024)) + up4(NV) + 14 up4(E_cap) + 512 ceil(E_cap / 256) + 512 with NV = (H + 1)(W + 1) and up4 =
     *    rounded up to a multiple of 4.  Its content before and after the launch means nothing.
     *    p3 = stream, 16-byte aligned, i4 = its capacity in bytes, a multiple of 4 (a stream of 0 bytes may be null): rings int32 [R][4]
     *    = object row k in p6 | index of the first vertex in the vertex array | vertices | unit edges L (the perimeter), followed
     *    directly by vertices uint32 [V] = x | y << 16.
     *    p7 = object table int32 [n][4], 16-byte aligned, written whatever it held: first ring | rings | first vertex | vertices; an
     *    absent or empty object gets (r, 0, v, 0) with r and v the running offsets.
     *    p4 = status int32 [4]: the stream's bytes 16 R + 4 V | error bits | R | E = the boundary edges of all listed objects (always
     *    valid).  With n == 0 only the status is written (all zero; p6 and p7 may be null).
     *    Error bit 1: the stream does not fit i4 -- NOTHING is written to p3 and the table's offsets are 0; the counts, R, E and the byte
     *    total stay valid.  Error bit 2: E > E_cap -- nothing is traced, words 0 and 2 are 0 and the table is all zero; word 3 says
     *    what was needed.
     *    Bounds: V <= 4 (H + 1)(W + 1), E <= 2 (H (W + 1) + (H + 1) W), R <= V / 4 (OpList.polygon_capacity).
     *    Determinism: integers only; every offset comes from a scan in a fixed order or from sums and minima whose result does not depend
     *    on the order of arrival: stream, table and status depend on the plane, the list and i5 alone -- not on i6, the launch shape or
     *    timing.
     *    The launcher refuses, each with its own message and before any launch: H, W < 1, H or W above 65535, (H + 1)(W + 1) >= 2^29 (the
     *    edge index has 31 bits), n outside 0 .. 255, a connectivity other than 4 or 8, i6 outside 0 .. 1, E_cap < 1, a negative capacity
     *    or one that is no multiple of 4, a null p2, p4, p5, p3 (with i4 > 0), p6 or p7 (with n > 0), p3, p5 or p7 not 16-byte aligned,
     *    p4 or p6 not 4-byte aligned, fewer scratch words than needed.
     * ABI 11, form added (the number stays 11; cutie_hip_build_flags() bit 8, value 256, says the form is present -- a library from before
     *    refuses such a descriptor as "unknown flags") -- the reference tool's 'rgba' output (gui/interactive_utils.py:218-229, saved by
     *    gui/resource_manager.py:158-161: the frame with the matte of the chosen objects as its alpha) and smooth grey planes as PNG;
     *    ResultSaver cutout= / png_codes='dynamic', process_video --cutout / --png-codes; DESIGN.md section 24:
     *  flags == 16384, a stage ON ITS OWN (16384 combined with any other flag stays the "unknown flags" error): the complete zlib stream of
     *    a PNG's IDAT chunk with scanline filters chosen per row and dynamic Huffman codes (kernels in png_photo.hip; the model:
     *    tests/png_photo_ref.py; the bytes are equal).  flags&8 is untouched: filter 0 and one fixed block, which suits id planes.
     *    p2 = first source uint8, i3 = its channels c0: 1 = a plane [H, W], 3 = packed pixels [H, W, 3]; i4 = its row stride in bytes
     *    (>= W c0).  p6 = optional uint8 plane [H, W] with row stride i5 >= W: the LAST channel.  i1 = H, i2 = W.  B = c0 + (p6 != 0) bytes
     *    per pixel = PNG colour type 0 (L), 4 (LA), 2 (RGB), 6 (RGBA) at 8 bits; the channels are interleaved while the rows are filtered.
     *    L = W B + 1 <= 16384 (CUTIE_PNG_PHOTO_ROW_LIMIT): every match distance lies inside DEFLATE's window and inside what RESIZE flags
     *    64 | 128 decode; LDS sets no lower limit.  i0, p0, p1, i6, i9 and the floats are unused.  The sources are READ ONLY.
     *    THE RULE (deterministic, independent of the launch shape):
     *    1 FILTER.  Raw byte j of a row: x; a = the byte B to the left (0 for j < B); b = the byte above (0 in the first row); c = the byte
     *      above a.  Residuals mod 256 of the filters 0 .. 4: x | x - a | x - b | x - ((a + b) >> 1) | x - paeth(a, b, c), paeth with
     *      p = a + b - c: a if |p - a| <= |p - b| and |p - a| <= |p - c|, else b if |p - b| <= |p - c|, else c.  The cost of a filter is
     *      the sum over the row of |residual read as int8| (0x80 counts 128); the lowest cost wins, ties go to the lower number.  The
     *      filtered row is the filter number followed by its W B residuals.
     *    2 TOKENS, on the filtered bytes f of a row, filter byte included; a token never crosses a row.  At byte i:
     *        n1 = the bytes from i on that equal their left neighbour in the row (0 at i = 0)        distance 1
     *        nB = the bytes from i on that equal the byte B before them in the row (0 for i < B; only B > 1)     distance B
     *        nL = the bytes from i on that equal the filtered byte one row up (0 in the first row)   distance L
     *      each counted up to 261 and no further.  n = max(n1, nB, nL); ties go to distance 1, then B, then L.  n < MINMATCH = 12: a
     *      literal, one byte.  Else a match of take(n) bytes at that distance, take(n) = n (n <= 258) | n - 3 (259, 260) | 258 (261),
     *      as flags&8.  (A distance-L match in a block's first row reaches into the block before: the window is continuous.)
     *    3 BLOCKS.  Rows r with r / 32 equal are one DEFLATE block (R = 32); the last block carries BFINAL.
     *    4 CODES, per block.  Counts of the literal/length symbols, end-of-block once, and of the distance symbols.  Code lengths of an
     *      alphabet: the symbols with a count sorted by (count, symbol) ascending; Huffman depths by the in-place two-queue merge over
     *      that list (Moffat & Katajainen; where a leaf and an inner node weigh the same the leaf is taken); depths above the limit (15;
     *      7 for the code-length code) are counted at the limit and, while the Kraft sum exceeds 1, one code leaves the limit and the
     *      longest shorter length that has a code gives one up to make two one level down; then the lengths, shortest first, go to the
     *      symbols from the END of the sorted list.  One symbol with a count: length 1 (inflate accepts the incomplete distance code);
     *      none: all zero, HDIST = 1 with one length 0.  Codes are canonical (RFC 1951 3.2.2).  HLIT, HDIST, HCLEN are the smallest legal
     *      values.  The HLIT + HDIST lengths form one sequence; at position i with value v and r equal values from i on: v == 0 and
     *      r >= 11: symbol 18 for min(r, 138) | v == 0 and r >= 3: symbol 17 for r | v != 0, i > 0, the value before is v and r >= 3:
     *      symbol 16 for min(r, 6) | else v itself.  The block is written with the FIXED codes (BTYPE 01) whenever that takes no more
     *      bits than the dynamic form, header and end-of-block included: so no block exceeds 9 bits per filtered byte + 10.
     *    5 zlib header 78 01, the blocks, the Adler-32 of the filtered bytes big-endian.
     *    p3 = stream uint8, 4-byte aligned, i7 = its capacity in bytes (rounded down to a multiple of 4).  ceil((9 H L + 10 ceil(H / 32))
     *    / 8) + 6 bytes hold any image (OpList.png_photo_capacity).  p4 = status int32 [4], written by the launch: 0 stream bytes, 1
     *    Adler-32, 2 error bits (1: the stream does not fit the capacity; NOTHING is written to p3 then -- with i7 < 4 it may be null --,
     *    [0] still says what it needs), 3 zero.  p5 = int32 scratch of i8 words, 16-byte aligned, i8 >= 4 H + 1024 ceil(H / 32) +
     *    up4(ceil(H L / 4)) + up4(ceil(H L / 2)) (OpList.png_photo_scratch_words); its content before and after means nothing.
     *    The launcher refuses, each with its own message and before any launch: H, W < 1, c0 other than 1 or 3, L above the row limit, a
     *    row stride below a row's bytes, 9 H L + 10 ceil(H / 32) + 64 >= 2^31 stream bits, a negative capacity, a null p2, p4, p5 or p3
     *    (with i7 >= 4), p3 or p4 not 4-byte aligned, p5 not 16-byte aligned, fewer scratch words than needed.
     *    cutie_amd/inference/utils/png.py assemble_image wraps the stream into a file (signature, IHDR, one IDAT, IEND).
     * ABI 11, form added (the number stays 11; cutie_hip_build_flags() bit 9, value 512, says the form is present -- a library from before
     *    refuses such a descriptor as "unknown flags") -- edge-aware refinement of the matte planes (not in the reference; ResultSaver
     *    matte_refine=, process_video --refine-matte / --refine-eps):
     *  flags == 32768, a stage ON ITS OWN (32768 combined with any other flag stays the "unknown flags" error): the colour guided filter
     *    (He, Sun, Tang, "Guided Image Filtering") of S uint8 planes under a uint8 RGB guide (kernels in guided.hip; the model:
     *    tests/guided_ref.py; the bytes are equal).  Every plane is fitted, per window, as an affine function of the guide's RGB and the
     *    fits of all windows that hold a pixel are averaged there: the planes' edges move onto the guide's.
     *    p2 = guide uint8 [H, W, 3], pixels packed, i4 = its row stride in bytes (>= 3 W), any alignment.  i1 = H, i2 = W, H, W >= 1 and
     *    H W < 2^31.  p6 = planes uint8 [S0, H, W], i9 = S0 >= 0, i5 = row stride (>= W), i6 = plane stride in bytes (>= (H - 1) i5 + W
     *    when S0 > 1), any alignment; p7 = an optional further plane uint8 [H, W] with row stride i10 (>= W), filtered as plane S0 (a
     *    matte in a buffer of its own).  S = S0 + (p7 != 0), 1 <= S <= CUTIE_GUIDED_MAX_PLANES.  The inputs are READ ONLY.
     *    i3 = radius r, 1 <= r <= CUTIE_GUIDED_MAX_RADIUS.  f0 = eps, 1e-6 <= eps <= 1, in units of the guide scaled to [0, 1].
     *    p3 = out uint8 [S, H, W] contiguous, any alignment; it overlaps neither an input nor the scratch.
     *    p5 = scratch int32, 4-byte aligned, of i8 + 2^31 * i7 words (i7, i8 >= 0): at least 4 S H W (OpList.guided_scratch_words), the
     *    coefficients.  Its content before and after the launch means nothing.  i0, p0, p1, p4 and the other floats are unused.
     *    THE ARITHMETIC (binding; I_c = the guide's channel c = 0, 1, 2 as an integer 0 .. 255, p = a plane's byte):
     *    WINDOW.  w(y, x) = the rows max(0, y - r) .. min(H - 1, y + r) and the columns max(0, x - r) .. min(W - 1, x + r): nothing exists
     *      outside the frame.  N = its pixel count, <= 129^2 = 16641.
     *    1 INTEGERS, exact, all sums over w(y, x).  Guide, once for all planes: S_c = sum I_c (3 values), S_cd = sum I_c I_d (6 values,
     *      c <= d).  Per plane: T = sum p, T_c = sum I_c p.  In int64: C_cd = N S_cd - S_c S_d, g_c = N T_c - S_c T.  (N S_cd <= 16641^2
     *      * 65025 ~ 1.8e13 < 2^53: every value converts to a double exactly, and no cancellation ever happens in floating point.)
     *    2 FLOAT64 per pixel, IEEE 754 binary64, every operation rounded on its own (no fused multiply-add), in this order:
     *        e = (((double)eps * 65025.0) * (double)N) * (double)N          (eps is the float of f0)
     *        m00 = (double)C_00 + e   m11 = (double)C_11 + e   m22 = (double)C_22 + e   m01 = (double)C_01   m02 = (double)C_02   m12 = (double)C_12
     *        a00 = m11 * m22 - m12 * m12      a01 = m02 * m12 - m01 * m22      a02 = m01 * m12 - m02 * m11
     *        a11 = m00 * m22 - m02 * m02      a12 = m01 * m02 - m00 * m12      a22 = m00 * m11 - m01 * m01
     *        det = (m00 * a00 + m01 * a01) + m02 * a02
     *      (the symmetric adjugate of M = C + eps 65025 N^2 Id and its determinant: once per pixel, shared by the S planes), then per plane
     *        a_0 = ((a00 * g_0 + a01 * g_1) + a02 * g_2) / det
     *        a_1 = ((a01 * g_0 + a11 * g_1) + a12 * g_2) / det
     *        a_2 = ((a02 * g_0 + a12 * g_1) + a22 * g_2) / det
     *        b   = ((double)T - ((a_0 * (double)S_0 + a_1 * (double)S_1) + a_2 * (double)S_2)) / (double)N
     *        A_c = sat_int32(rint(a_c * 1048576.0))     B = sat_int32(rint(b * 4096.0))       rint: round half to even
     *      (a term "x * y - z * w" is two products and a difference.)  |a| <= sigma_p / (2 sqrt(eps)) <= 250 at eps = 1e-6, so |A| <=
     *      2.7e8; |b| <= 255 (1 + 250 sqrt(3)), so |B| <= 4.6e8: both fit an int32, the saturation is a guard and not a path.  float64
     *      because a grey guide (R = G = B) makes C rank 1: a float32 adjugate at eps = 1e-6 is wrong by tens of grey levels there.
     *    3 INTEGERS, exact: sum A_c and sum B over w(y, x), in int64 (the coefficients of the windows centred in w(y, x)).
     *    4 FLOAT64, as in 2:
     *        q = (((((double)sum A_0 * (double)I_0 + (double)sum A_1 * (double)I_1) + (double)sum A_2 * (double)I_2) * 2^-20) + (double)sum B * 2^-12) / (double)N
     *        out = (uint8)min(max(rint(q), 0), 255)        with I_c the guide at (y, x)
     *    Consequences: a CONSTANT plane comes back unchanged, exactly (g_c = 0 as integers, so a = 0, b = the constant, B = 4096 times
     *    it, q = it).  Every order-dependent sum is an integer sum and the float64 steps are per pixel: the bytes depend on the inputs, r
     *    and eps alone -- not on the launch shape, the tiling, the summation order or timing; two runs give the same bytes.  (The
     *    kernels slide integer sums along columns and take differences of prefix sums modulo 2^32: exact, a window sum is below 2^32.)
     *    The launcher refuses, each with its own message and before any launch: H, W < 1 or H W >= 2^31, a radius outside 1 ..
     *    CUTIE_GUIDED_MAX_RADIUS, an eps outside 1e-6 .. 1 (NaN included), S outside 1 .. CUTIE_GUIDED_MAX_PLANES or a negative S0, a
     *    null p2, p3, p5 or p6 (with S0 > 0), a guide row stride below 3 W, plane strides below a row's or a plane's bytes, p5 not 4-byte
     *    aligned, a negative scratch size, fewer scratch words than 4 S H W, an output or a scratch that overlaps an input or each other.
     * ABI 11, form added (the number stays 11; cutie_hip_build_flags() bit 10, value 1024, says the form is present -- a library from
     *    before refuses such a descriptor as "unknown flags") -- redacted frames and background blur (not in the reference; ResultSaver
     *    redact=, process_video --redact):
     *  flags == 65536, a stage ON ITS OWN (65536 combined with any other flag stays the "unknown flags" error): the frame with an effect
     *    -- blur, pixelate or a fill colour -- blended over it under a weight plane (kernels in redact.hip; the model: tests/redact_ref.py;
     *    the bytes are equal).
     *    p2 = frame uint8 [H, W, 3], pixels packed, i4 = its row stride in bytes (>= 3 W), any alignment.  p6 = weight plane w uint8
     *    [H, W], i5 = its row stride (>= W), any alignment: 0 keeps the frame, 255 takes the effect, values between blend.  Both are READ
     *    ONLY.  i1 = H, i2 = W, H, W >= 1 and H W < 2^31.  i6 = mode: 0 blur, 1 pixelate, 2 fill.  i3 = strength: the radius r of blur,
     *    1 <= r <= CUTIE_REDACT_MAX_RADIUS; the cell size c of pixelate, 2 <= c <= CUTIE_REDACT_MAX_CELL; unused by fill.  i10 = the fill
     *    colour, R | G << 8 | B << 16 (0 .. 2^24 - 1; read by fill only).  i9 = the invert bit, 0 or 1.
     *    p3 = out uint8 [H, W, 3] contiguous, any alignment; it overlaps neither an input nor the scratch.
     *    p5 = scratch int32, 4-byte aligned, of i8 + 2^31 * i7 words (i7, i8 >= 0), at least OpList.redact_scratch_words(mode, H, W):
     *    blur 2 ceil(3 H W / 4) (two uint8 RGB images), pixelate ceil(H / c) 3 W + ceil(3 ceil(H / c) ceil(W / c) / 4) (column sums and
     *    the cells' bytes), fill 1 (never touched; the pointer is not null).  Its content before and after the launch means nothing.
     *    i0, p0, p1, p4, p7 and the floats are unused.
     *    THE ARITHMETIC (binding; integers only; f = the frame's byte, every channel on its own, "/" = floor division of non-negative
     *    integers):
     *    BLUR.  Exactly three passes.  One pass maps a uint8 image a to a': with w(y, x) = the rows max(0, y - r) .. min(H - 1, y + r) and
     *      the columns max(0, x - r) .. min(W - 1, x + r) -- nothing exists outside the frame --, N its pixel count (<= 129^2 = 16641)
     *      and S the sum of a over it, a'(y, x) = (2 S + N) / (2 N): ONE 2-D window mean rounded once, not a rounded row mean followed by
     *      a rounded column mean.  The effect e is the third pass's output (three boxes of radius r: a Gaussian of sigma about
     *      sqrt(r (r + 1))).  S <= 255 * 16641 < 2^23: the kernels slide sums and take prefix differences modulo 2^32, exactly.
     *    PIXELATE.  Cell (Y, X) holds the rows Y c .. min(H, (Y + 1) c) - 1 and the columns X c .. min(W, (X + 1) c) - 1: anchored at the
     *      frame's origin, cut by its far edges.  With n the cell's pixel count and S its sum, e = (2 S + n) / (2 n) for every pixel of it.
     *    FILL.  e = the colour's byte.
     *    BLEND.  w' = w, or 255 - w with the invert bit; out = (w' e + (255 - w') f + 127) / 255.
     *    Consequences: w' == 0 returns the frame's byte and w' == 255 returns e, both exactly; a CONSTANT frame comes back unchanged under
     *    blur and pixelate for every w.  Every order-dependent sum is an integer sum: the bytes depend on the inputs, the mode and the
     *    strength alone -- not on the launch shape, the tiling or timing; two runs give the same bytes.
     *    The launcher refuses, each with its own message and before any launch: H, W < 1 or H W >= 2^31, an unknown mode, a radius outside
     *    1 .. CUTIE_REDACT_MAX_RADIUS, a cell outside 2 .. CUTIE_REDACT_MAX_CELL, an invert word other than 0 or 1 or a colour beyond three
     *    bytes, a null p2, p6, p3 or p5, a frame row stride below 3 W, a weight row stride below W, p5 not 4-byte aligned, a negative
     *    scratch size, fewer scratch words than needed, an output or a scratch that overlaps an input or each other. */
    CUTIE_OP_PROB_TO_ID = 36,
    /* RESIZE: F.interpolate(x, size=(OH,OW)) -- the max_internal_size path of InferenceCore.step (inference_core.py:206-228,
     * 321-326): bilinear align_corners=False without antialias (flags&1 == 0) or nearest-exact (flags&1, index masks).
     * p0=src f32 (C planes of H x W, plane stride i5, row stride i6) p1=dst f32 [C,OH,OW]   i: 0 C 1 H 2 W 3 OH 4 OW 5 6
     * ABI 5 -- frame ingest (video_reader.py:42-46,97-98: ToTensor + Resize of the dataset frames; cutie_amd/inference/data/device_ingest.py),
     *    kernels in ingest.hip; flags&1 together with flags&2 or flags&4 is an error:
     *  flags&2: antialiased bilinear, F.interpolate(mode='bilinear', align_corners=False, antialias=True) = torch's separable triangle filter
     *    (_upsample_bilinear2d_aa): horizontal pass into the scratch, then vertical pass, taps summed in ascending order in fp32.
     *    The tap table is computed on the HOST, once per geometry, and passed in (cutie_amd/ops.py aa_taps / resize_aa_table: it rounds
     *    center, support and weights exactly as torch's CPU kernel does for float input, so the tap ranges and weights are torch's):
     *    p2 = int32 [OW + OH][i7 + 2]: row = first tap, tap count, i7 fp32 weights (as bits); rows 0..OW-1 the horizontal pass, then OH rows
     *    of the vertical pass (an axis whose size does not change is one tap of weight 1).  p3 = f32 scratch [C, H, OW].  i7 = taps per row.
     *    dst and scratch 16-byte aligned.
     *  flags&4: p0 = u8 [H, W, C] interleaved (what PIL / numpy decode), row stride i6 BYTES (>= W*C), pixel stride C (i5 ignored); every
     *    value becomes v / 255.0f correctly rounded = u8.float().div_(255.0), bit for bit.  Without flags&2: ToTensor alone, OH == H, OW == W.
     * ABI 6 -- baseline JPEG decode on the GPU (ingest='device-decode'; kernels in jpeg.hip): flags 8 / 16 / 32 are the three stages and
     *    may be set together (they run in that order); with any of them flags 1 / 2 / 4 are an error and the RESIZE fields above do not apply.
     *    p0 = the packet (uint8, 4-byte aligned), built by cutie_amd/inference/data/jpeg.py: header, segment / chunk / component tables,
     *    quant and Huffman tables, destuffed entropy data.  Every result equals libjpeg's (PIL's Image.open(...).convert('RGB')) bit for bit.
     *    i: 0 chunks 1 segments 2 blocks 3 chunk bits 4 sync rounds 5 packet bytes 6 plane bytes 7 H 8 W 9 work words 10 components
     *       11 rgb row stride (bytes, >= 3 W) -- copied from the packet header by ops.py OpList.jpeg_*.
     *  flags&8 Huffman: self-synchronising speculative decode, one thread per chunk of i3 bits; i4 sync rounds, then any segment that
     *    has not synchronised is decoded serially.  p1 = int32 work (8-byte aligned, >= 10 * i0 + (i4 + 1) * i1 words: chunk exits,
     *    block counts and DC sums with their scans, per-round flags), p2 = int16 coef [i2][64] (natural order, quantised as in the file, absolute DC),
     *    p3 = int32 status [4], cleared by the launch: 0 error bits (1 bad Huffman code, 2 data ends early -- where libjpeg goes on
     *    with zeros and a warning; nonzero = the frame is bad), 1 sync rounds used (max over segments; i4 + 1 = serial), 2 serial segments.
     *  flags&16 IDCT: libjpeg's ISLOW (jidctint.c: CONST_BITS 13, PASS1_BITS 2, DESCALE rounding, 64-bit intermediates, the range-limit
     *    table with its 10-bit wrap), dequantising p2 with the packet's tables -> p4 = uint8 planes (i6 bytes, 8-byte aligned): per
     *    component blocks_w * 8 wide, whole blocks.
     *  flags&32 colour: libjpeg's fancy upsampling (h2v1 / h2v2 where the chroma width is > 2, h1v2 always; else replication) and its
     *    fixed-point YCbCr -> RGB tables (SCALEBITS 16); one component is replicated -> p5 = uint8 [H, W, 3], row stride i11 bytes:
     *    the source of RESIZE flags 4 / 6.
     * ABI 11, forms added (the number stays 11; cutie_hip_build_flags() bit 2, value 4, says the forms are present -- a library from before
     *    would read such a descriptor as a one-frame decode, so the callers ask first: cutie_amd/_lib.py has_jpeg_batch) -- flags&256
     *    "batch": the stages above (flags 8 / 16 / 32, any of them, in that order; every other flag is an error) over N images, every pass
     *    ONE launch over all of them (device_ingest.jpegs_to_device, --decode-batch): a frame's Huffman passes take about as long for 16
     *    frames as for one, so a window of frames pays the chain once.
     *    i: 0 N images (1 .. 65535)  1 bytes of p0  2 int32 words of p2  3 int16 elements of p3  4 bytes of p4  5 bytes of p5
     *       6 sync rounds  7 / 8 / 9 / 10 the largest chunk / segment / block / pixel (H * W) count of the batch: the grids.
     *    p0 = packets uint8: the unchanged packets of jpeg.py, each starting at a multiple of 16.  p1 = table int32 [N][8], per image:
     *    0 byte offset of its packet in p0 (multiple of 16)  1 int32-word offset of its work area in p2 (even: 8-byte aligned)  2 int16-element
     *    offset of its coefficient blocks in p3 (multiple of 8: 16-byte aligned)  3 byte offset of its planes in p4 (multiple of 8)
     *    4 byte offset of its rgb in p5 (multiple of 16)  5 its packet bytes  6 its rgb row stride in bytes (>= 3 W)  7 zero.  Every other
     *    geometry is read from the image's own packet header.  p2 = work int32 (8-byte aligned; per image 10 * chunks + (i6 + 1) *
     *    segments words, as above), p3 = coef int16 (16-byte aligned), p4 = planes uint8 (8-byte aligned), p5 = rgb uint8 (16-byte aligned),
     *    p6 = status int32 [N][4]: row k means for image k what status[4] means above, cleared by the launch with flags&8 (one memset;
     *    the per-round flags and the coefficients of all images are cleared by one kernel -- their regions lie apart -- so the number
     *    of memsets does not depend on N).  p0, p1, p6 16-byte aligned.  ops.py OpList.jpeg_layout lays the buffers out.
     *    Table and headers are device data: every kernel checks the image's row and header against i1 .. i10 before it reads or writes
     *    anything else of the image -- the magic word and the header's byte count against the row; every section offset plus its size
     *    inside the packet; the counts (components 1 | 3, 1 .. 10 blocks per MCU, 1 .. 6 tables, chunk bits >= 64, sampling 1 | 2) and
     *    chunks / segments / blocks / pixels against i7 .. i10; offsets plus sizes inside each buffer and their alignment; and 10 * chunks
     *    + (i6 + 1) * segments against the words between the row's work offset and the next row's (i2 for the last row), i.e. the header's
     *    chunk count against what the host laid out.  An image that fails gets error bit 4 ("bad table or header") in its status[0] and
     *    every stage skips it; the other images are not affected, and no read or write leaves an image's own extents whatever the
     *    entropy data holds (the section tables inside a packet are the parser's, as in the one-frame form).  Grids: the image is
     *    blockIdx.y (the scan: one workgroup per image), sized by i7 .. i10; workgroups past an image's own count return.
     * ABI 11, forms added (the number stays 11; cutie_hip_build_flags() bit 1 says the forms are present -- a library from before would run
     *    such a descriptor as a plain RESIZE, so the callers ask first) -- mask PNGs decoded on the GPU (SequenceScorer gt_decode='device',
     *    score_masks --decode device; kernels in png_dec.hip, their serial core in png_inflate_core.h; the Python model: tests/png_dec_ref.py):
     *    flags 64 / 128 are the two stages and may be set together (they run in that order); with either of them every other flag is an
     *    error and the RESIZE fields above do not apply.  ONE launch takes i0 = N images (1 .. 65535), one wave64 per image.
     *    p0 = packets uint8 (i1 bytes), built by cutie_amd/inference/data/png_packet.py: per image 8 little-endian int32 words -- magic
     *    'PNGD', W, H, bit depth (1 | 2 | 4 | 8), channels (1; 3 = RGB at 8 bits), bytes per filtered row (<= 16384), stream bytes, inflated
     *    bytes = H * (rowbytes + 1) -- then the zlib stream (all IDAT chunks joined).  p1 = table int32 [N][4]: per image the byte offset of
     *    its packet in p0, of its inflated rows in p2 and of its pixels in p3 (the first two multiples of 16), 0.  p2 = inflate buffer
     *    uint8 (i2 bytes), p3 = output uint8 (i3 bytes; flags&128 only), p4 = status int32 [N][4].  p0, p1, p2, p4 16-byte aligned.
     *    Header and table are device data: both kernels check them against i1 .. i3 before they read anything else.
     *  flags&64 inflate (RFC 1950 / 1951): stored, fixed and dynamic blocks, any number of them; code tables per block in LDS; one lane
     *    decodes up to 64 tokens into an LDS queue, the wave executes it (literals scattered, a match copied by all lanes as
     *    out[pos + i] = out[pos - dist + i % dist], the window being the output itself); Adler-32 of the output against the trailer.
     *    status, cleared by the launch: 0 error bits -- 1 reserved block type, 2 over-subscribed / incomplete code lengths, 4 invalid
     *    symbol, 8 distance beyond the bytes produced, 16 stream ends early, 32 output exceeds or falls short of the inflated length,
     *    64 stored LEN != ~NLEN, 128 Adler-32 mismatch, 256 filter byte above 4 (set by flags&128), 512 bad packet header / table entry /
     *    zlib header; 1 bytes produced, 2 blocks, 3 tokens.  The first error ends the image's decode; the other images are not affected.
     *    Every stream read, output write and match source is bounds-checked when the token is decoded; the work is bounded by
     *    8 * stream bytes + inflated bytes whatever the bytes are (png_inflate_core.h has the argument).
     *  flags&128 unfilter + unpack: images without an error bit; rows in order, two rows in LDS; filters 0 / 2 lane-parallel, 1 a wave prefix
     *    sum mod 256 per channel (filter unit 1 byte, 3 for RGB; packed depths on the packed bytes), 3 / 4 one serial lane; pixels of
     *    1 / 2 / 4 bits unpacked MSB first -> uint8 [H, W], RGB -> uint8 [H, W, 3], at the image's offset in p3: np.array(Image.open(f)). */
    CUTIE_OP_RESIZE = 37,
    /* FLIP_W: dst = f0 * flip_last_dim(src) + f1 * dst   -- torch.flip(x, dims=[-1]) of the flip_aug path and the averaging
     * of the two passes (inference_core.py:162-165,234-235,303-305).  src and dst must not overlap.
     * p0=src f32 [rows, W] (row stride i2) p1=dst f32 [rows, W] (row stride i3)   i: 0 rows 1 W 2 3   f: 0 alpha 1 beta */
    CUTIE_OP_FLIP_W = 38,
    /* AREA_DOWN3: three AREA_DOWNs in one launch (SensoryUpdater's area poolings of g8 / g4 / logits, modules.py:59-60).
     * segment q = 0..2: p[2q]=x p[2q+1]=y, i[8q..8q+7] = B H W C ldx ldy r Cz as in AREA_DOWN, flags bit q: f32 input;
     * flags&8: the bodies with a run-time r also for r = 2, 4 (A/B switch; default: r as a compile-time constant, all taps in flight -- same bits) */
    CUTIE_OP_AREA_DOWN3 = 39,
    /* QFFN: the FFN of a QueryTransformerBlock in one launch (transformer_layers.py:101-118: x + linear2(relu(linear1(norm(x))))),
     * split over FF / i2 slices of the hidden layer: grid (FF / i2, K).  Input rows as a sum (the self-attention out-projection):
     * x_eff = p0 (f32 [K*16,256], the residual) + p11 (bias f32 [256], may be 0) + p10 / 2^32 (p10 = int64 [K*16, 256], may be 0)
     * p1 = x_out f32 [K*16,256] (x_eff, written once: the residual of the FFN)  p2/p3 = LayerNorm gamma/beta
     * p4 = W1 bf16 [FF,256] p5 = b1 f32 [FF]  p6 = W2 bf16 [256,FF]
     * p7 = int64 [K*16, 256]: += relu(LN(x_eff) W1^T + b1) W2^T in fixed point (x 2^32), slice by slice (cleared by the caller).
     * linear2's bias and the residual x_out are added by the consumer (flags&4 of the attention ops).
     * i: 0 rows (K*16) 1 FF 2 hidden columns per block (64 | 128; 0: 64) */
    CUTIE_OP_QFFN = 40,
    /* STEM: IMG_PREP + the 7x7 / stride-2 / pad-3 conv with folded BN (Cin 3 + mask + others padded to 8, Cout 64) + 3x3 / stride-2 /
     * pad-1 max pool in one launch (resnet.py conv1, bn1, relu, maxpool; big_modules.py:30-33, 95-100): same rounding points as the
     * three ops (bf16 after the conv, max of bf16 values).
     * p0=image f32 [3,h0,w0] p1=masks f32 [K,H,W] (0: none, K = 1) p2=packed weights bf16 [64,Kpad] (k = (kh*7+kw)*8 + c)
     * p3=bias f32 [64] p4=y bf16 [K,H/4,W/4,64]   i: 0 h0 1 w0 2 H 3 W (multiples of 16) 4 pad_left 5 pad_top 6 K 7 Kpad
     * f: 0-2 mean 3-5 std   flags&1: ReLU (before or after the pool: the same)
     * ABI 4: i8 > 1 = frames per launch (<= 12; grid.y): frame f > 0 reads the image at p[4 + f] (p5 .. p15) and the masks at p1 + f * i9 floats and
     *      writes y + f * K*(H/4)*(W/4)*64 -- the frames of a look-ahead encoder window, or the clips of a lock-step group (one image + K masks each),
     *      in one launch that fills the chip (a 480p frame is 210 blocks: a partial round of its own); per frame exactly the one-frame launch
     * Mixed form: i10 != 0 = the object counts of the i8 clips (3-bit fields; needs p1; i6 = the largest count = grid.z; i9 unused): clip f has
     *      K_f objects, its masks are the planes p1 + (start_f + f) * H*W .. (p1 = the first object plane of a mixed group's probability
     *      tensor) and it writes y + start_f * (H/4)*(W/4)*64; blocks with z >= K_f return */
    CUTIE_OP_STEM = 41,
    /* BANK_WRITE: the contiguous copies and fills of one memory insertion (memory_manager.py:210-296, kv_memory_store.py:55-149: the
     * reference torch.cat's every tensor of the bank; here a frame's keys / shrinkage / selection / per-object values go to their slot)
     * in ONE launch.  Up to 6 copies: p[2s] = src, p[2s+1] = dst, i[s] = 32-bit words (0: unused), s = 0..5; up to 2 fills:
     * p[12+t] = dst, i[6+t] = words, i[8+t] = the 32-bit pattern, t = 0..1.  Sources and destinations must not overlap. */
    CUTIE_OP_BANK_WRITE = 42,
    CUTIE_OP__COUNT
};

/* Execute n descriptors in order on `stream`.  Returns 0 or a negative error code. */
int cutie_exec(const cutie_op* ops, int n, void* stream);
/* Single-op entry (used by the kernel unit tests). */
int cutie_exec_one(const cutie_op* op, void* stream);
/* HIP-graph capture of a plan: returns an opaque handle (0 on failure); replay with cutie_graph_launch. */
void* cutie_graph_capture(const cutie_op* ops, int n, void* stream);
int cutie_graph_launch(void* graph, void* stream);
void cutie_graph_destroy(void* graph);
/* Timing helper: runs the plan `iters` times between two hipEvents on `stream`, returns mean ms (<0 on error).
 * bench.py uses it to time the dominant kernel on the launch stream (roofline.achieved). */
float cutie_time_ops(const cutie_op* ops, int n, int iters, void* stream);
const char* cutie_hip_last_error(void);
int cutie_hip_abi_version(void);
int cutie_op_struct_size(void);
/* bit 0: the library was built with -DCUTIE_DIAG (make DIAG=1): measured-and-lost kernel variants (ATTN_P2Q flags&32) are present.
 * The product library returns 0 and rejects those descriptors.
 * bit 1 (value 2): RESIZE flags 64 / 128, the PNG decode stages, are present.  bit 2 (value 4): RESIZE flags 256, the batch forms of the
 * JPEG decode stages, are present (both came without a new ABI number).  bit 3 (value 8): the mixed forms of the lock-step ops are present.
 * bit 4 (value 16): PROB_TO_ID flags == 1024, the track statistics, is present.  bit 5 (value 32): PROB_TO_ID flags == 2048, the region
 * filter, is present.  bit 6 (value 64): PROB_TO_ID flags == 4096, the distance transform and its bands, is present.  bit 7 (value 128):
 * PROB_TO_ID flags == 8192, the polygon trace, is present.  bit 8 (value 256): PROB_TO_ID flags == 16384, the PNG stream with scanline
 * filters and dynamic Huffman codes, is present.  bit 9 (value 512): PROB_TO_ID flags == 32768, the colour guided filter, is present.
 * bit 10 (value 1024): PROB_TO_ID flags == 65536, the redacted frame (blur, pixelate, fill under a weight plane), is present. */
int cutie_hip_build_flags(void);

#ifdef __cplusplus
}
#endif
#endif
