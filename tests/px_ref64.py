"""Float64 references of the mask decoder's pixel kernels (csrc/elementwise.hip: IMG_PREP, MAXPOOL, UPSAMPLE2X_ADD, AREA_DOWN / AREA_DOWN3,
MASK_DOWN, GAP, ECA_APPLY, GRU, SEG_AGG, UP4_SOFTMAX, MASK_MERGE, AGG_SOFTMAX) with per-element error bounds, the checks built on them and the
case list shared by tests/test_px_ref64_cpu.py (the interpreter on the host) and tests/test_gpu_px_ref64.py (the HIP kernels).
TEST INFRASTRUCTURE ONLY.

Independent of tests/mock_exec.py and of the kernels: every reference reads the buffers ONE launch reads and applies the op contracts of
include/cutie_hip.h and the formulas of oracle/net.py (aggregate, _gru, _others, the _ca_block arithmetic, segment's interpolations) in
float64.  Each function returns {name: (y64, bound)}; an element whose bound is 0 is an EXACT output and is compared by value.  No bound is
fitted to what a kernel returns.  They rest on: u = 2^-24 (ref64.U32; the build uses -ffp-contract=off and no fast-math, so every fp32
+ - x / is ONE rounding to nearest), ub = 2^-8 (ref64.U_BF16), gamma_n = n u / (1 - n u) (+ n 2^-53 for the float64 sum itself; a sum of n
terms in ANY order is within gamma_n sum |terms|: Higham, Lemma 3.1) and FTZ = 2^-126 per rounding step for flushed denormals.

Transcendentals.  sigmoidf_ = 1 / (1 + __expf(-x)), the fast exp: |err| <= (|x| / 4 + 4) u absolute (the accounting of ref64.py and
attn_ref64.py: the rounding of x log2 e is a relative |x| u of the exponential, v_exp_f32, the add and the reciprocal an ulp each, all of it
through sigma' <= 1 / 4).  expf (the seg tail): 2 ulp = 4 u relative (aff_ref64.py).  logf and tanhf: the limits
of the OpenCL full profile that the device library (OCML) is built to meet: log <= 3 ulp = LOG_ULP, tanh <= 5 ulp = TANH_ULP (OpenCL C
specification, "Relative error as ULPs"); one ulp of a result y is at most 2^-23 |y| = 2 u |y|.

Bilinear maps (``up_coords`` / ``bilinear_ref``; torch area_pixel_compute_source_index, align_corners = False): src = max((o + 1/2) s - 1/2,
0), i0 = floor(src), i1 = min(i0 + 1, n - 1), lam = src - i0.  At s = 1/2 lam is 0, 1/4 or 3/4, at s = 1/4 it is 0 or an odd multiple of
1/8: ly, lx, 1 - ly, 1 - lx are exact dyadics and so are their products w00 .. w11, multiples of 2^-4 (2^-6) in [0, 1]
(test_px_ref64_cpu.py asserts that the float64 weights survive a cast to fp32 unchanged).  Roundings come from the four value x weight
products and the adds only: v = sum w a within gamma_4 sum |w a| (+ the weighted input errors), with a fifth term (UPSAMPLE2X_ADD's skip
value) gamma_5.

UPSAMPLE2X_ADD: gamma_5 (sum |w g| + |skip|), then the bf16 store, ub (|y| + e).  The skip map of object b is that of its group: b / Kg
(skip groups), the clip that holds b (mixed counts), map 0 otherwise.
AREA_DOWN / AREA_DOWN3: r^2 terms summed in some order, times inv = fl(1 / r^2) (its own rounding where r^2 is no power of two, and the
product's): gamma_(r^2 + 1) mean |x|, then the bf16 store.  The f32 form fills the channels [C, Cz) with exact zeros.
IMG_PREP: (x - m) / s with the fp32 m, s of the descriptor: two roundings, gamma_2 |v|, then bf16; padding pixels hold (0 - m) / s.  Channel
3 is bf16(mask), exact; channel 4 = clamp(sum_j m_j - m_k, 0, 1): K roundings on a magnitude of sum |m| + |m_k|, through a clamp of
Lipschitz constant 1 (no hull is needed at 0 and 1: |clamp(a') - clamp(a)| <= |a' - a| everywhere), then bf16; channels 5 .. 7 are exact
zeros, and so are 3, 4 without masks.
MAXPOOL: a selection of inputs over the taps inside the map, started from 0 with ReLU and from -inf without: exact.
MASK_DOWN: m16 = the mean of 256 values, gamma_256 mean |m| whatever the lane order (the division by 256 is exact); pair[0] = bf16(m16);
pair[1] = clamp(sum_k a_k - a, 0, 1) from the COMPUTED means: the means' own errors add up, K + 1 roundings on sum |a| + |a|, Lipschitz 1,
bf16.  With K = 1 the difference is a - a: exactly 0.  Channels 2 .. 7 are exact zeros; channels 8 .. of a 64-pitch pair are not written.
``mask_down_ref`` takes an error of its input, so the same function bounds UP4_SOFTMAX's mask-down outputs from the raw logits.
GAP: part[b][chunk][c] = the sum of the chunk's <= 64 bf16 values: gamma_64 sum |x|; y = the sum of all HW values times fl(1 / HW):
gamma_(HW + 2) mean |x| (the bound of the whole chain GAP -> ECA is this gamma_HW over exact bf16 values; ECA_APPLY itself is referenced
from the partials IT reads, which is tighter).
ECA_APPLY: mean_c from the partials as read (nchunk terms, times fl(1 / HW): gamma_(nchunk + 2)) or from the int64 fixed-point sums
(units of 2^-24, the sum of ref64.gap_fixed(v) * 16; the conversion to double and the scaling by 2^-24 are exact,
then one rounding to fp32, fl(1 / HW) and the product: gamma_3 |mean|).  a_c = the five-tap channel convolution with zero padding:
sum |wk| e_mean + gamma_5 sum |wk mean|.  s = sigmoidf_(a): e_a / 4 + (|a| / 4 + 4) u.  y = x s + r: |x| e_s + gamma_2 (|x| s + |r|),
then bf16.  gap_out = mean_c (fp32, no further rounding).  The head reads the STORED bf16 y: ``eca_head_ref`` sums relu(y) w over the
interval [bf16(y64 - e), bf16(y64 + e)] of every channel (rounding is monotone, so the stored value lies in it: the hull over both
neighbours wherever y64 is within its bound of a rounding point, a single value elsewhere), plus gamma_514 (sum |relu(y) w| + |bias|) for
256 products, their adds, the lane reduction and the bias.  Given the stored y itself (the GPU tests do both) the interval is a point.
GRU: f = sigmoidf_, u = sigmoidf_, n = tanhf (TANH_ULP); h' = f h (1 - u) + u n: three products and the subtraction on the first term
(gamma_4), one product on the second (with the final add gamma_2), the operands' errors carried with their perturbed magnitudes; the bf16
shadow adds ub (|h'| + e).  The reference is computed from a copy of h taken before the launch (the kernel updates h in place).
SEG_AGG (``agg_ref``, ``sigmoid_exact_err``): p = 1 / (1 + expf(-x)) with E = e^-x: expf gives p q 4 u; s = fl(1 + E) is off by at most
min(u s, E, 1) (1 and E are fp32 numbers themselves), a relative min(u, q, p) of p; the division is one rounding, and exact where s == 1
(E < 2^-24).  So a saturated sigmoid is off by E, not by u: at x = 25 e_p = 1.4e-11.  q = 1 - p is exact for p >= 1/2 (Sterbenz), else one
rounding of at most min(u q, p).  bg = prod q_k in object order, as every kernel multiplies it up (``prob_bg_ref``): each step carries the
error so far and rounds once, by at most u of the product and at most what either factor lacks to 1 -- so the background of a pixel
where every object is far below 0 stays within the sum of the p_k of 1, beyond the clamp.
clamp_logit (``clamp_logit_ref``): p is clamped to the FP32 constants LO32 = float32(1e-7) and HI32 = float32(1 - 1e-7) = 1 - 2^-23 (the
oracle clamps a float32 tensor with the same two numbers); logit(q) = log(q / (1 - q)) is increasing, so an input within e_p of p gives a
result between logit(clamp(p - e_p)) and logit(clamp(p + e_p)): the bound is the distance from logit(clamp(p)) to the farther end of that
hull -- on a clamp it collapses to the constant, next to a clamp either side is legal, away from the clamps it is e_p / (p (1 - p)) --
plus the evaluation itself: 1 - q (exact for q >= 1/2), the division (together 2 u of the ratio, 2 u absolute of its logarithm) and logf,
LOG_ULP ulp of the result.  Off the clamps the bound GROWS as p -> 1: with an e_p of 2 u = 1.2e-7 it is 4.8e-5 at a logit of 6 and
2.0e-2 at 12 (the sigmoid's own e_p is p q 4 u + 2 u p there); at 16 (1 - p = 1.1e-7, just beyond the clamp at 15.94, where 1 + E still rounds
to 1 + 2^-23 or to 1) the hull reaches back from the clamp constant to logit(p - e_p).  That is the model's own fp32 formulation (p carries
2^-24 absolute next to 1, the logit divides it by 1 - p), not looseness.  Beyond |x| = 17 or so -- where real frames sit -- e_p is E
itself, p +- e_p and bg + e_bg stay beyond the clamp constants, and the bound IS LOG_ULP ulp of a constant plus the 2 u of the ratio: 5.8e-6 at
+-15.94 (test_px_ref64_cpu.py asserts it at |x| = 25, and 1e-5 on the fused probabilities there).
Softmax over P planes (``softmax_ref``): the maximum is exact; d = v - mx takes one rounding, a relative |d| u of its exponential; expf
4 u; the sum of P positive terms gamma_P; inv = 1 / sum and the product two roundings: rel = (1 + a)(1 + u)^2 / (1 - b) - 1 with
a = (|d| + 4) u, b = max a + gamma_P.  Errors e_v of the logits themselves: w_c = 1 / (1 + sum_{j != c} e^(v_j - v_c)), and every exponent
moves by at most e_j + e_c, so w_c lies between the two values at +-(e_j + e_c): a plane that dominates its pixel moves by the OTHER planes'
weights times their errors, a plane of negligible weight by a factor e^(+-(e_j + e_c)) of that weight.  UP4_SOFTMAX from aggregated logits (the two-launch form) has e_v = gamma_4 sum |w a|; the fused forms carry the
SEG_AGG bounds of their four source pixels through the weights.  logits_up = v with e_v.
AGG_SOFTMAX: bg = prod (1 - p_k) as in SEG_AGG (the planes are exact inputs), clamp_logit of bg and of every plane, softmax over K + 1.
MASK_MERGE: every plane is a copy of an input value or 0 / 1: exact."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from aff_ref64 import Bufs, bits, gamma, SENT_F                       # noqa: F401  (re-exported for the tests)
from ref64 import FTZ, U32, U64, U_BF16, check_bound, gap_fixed
from cutie_amd import ops as O

F64, F32, BF16, I32, I64 = torch.float64, torch.float32, torch.bfloat16, torch.int32, torch.int64
LOG_ULP, TANH_ULP = 3, 5
LO32 = float(np.float32(1e-7))
HI32 = float(np.float32(1.0) - np.float32(1e-7))
assert HI32 == 1 - 2.0 ** -23
NAN = float('nan')


def d64(t):
    return t.detach().cpu().to(F64)


def bf16_round(t):
    """float64 -> the nearest bf16 (ties to even) as float64; through fp32 (double rounding needs a float64 within 2^-29 relative of a bf16
    tie that is itself no fp32 number: none of the values here is built that way, and the hull users widen by the bound first)."""
    return t.to(F32).to(BF16).to(F64)


def with_bf16_store(y, e):
    return e + U_BF16 * (y.abs() + e) + FTZ


def chk(got, ref, what=''):
    """Every element of `got` within its bound of ref = (y64, bound); bound == 0: equal in value.  Returns the worst |err| / bound."""
    y, b = ref
    assert tuple(got.shape) == tuple(y.shape), (what, tuple(got.shape), tuple(y.shape))
    n = y.shape[-1] if y.dim() > 1 else 1
    b = torch.where(b == 0, torch.full_like(b, 5e-324), b)
    return check_bound(d64(got).reshape(-1, n), y.reshape(-1, n), b.reshape(-1, n), what=what)


def all_finite(refs):
    return all(bool(torch.isfinite(y).all()) and bool(torch.isfinite(b).all()) and bool((b >= 0).all()) for y, b in refs.values())


# ---- bilinear ---------------------------------------------------------------------------------------------------------------------------
def up_coords(n_out, n_in, scale):
    o = torch.arange(n_out, dtype=F64)
    src = ((o + 0.5) * scale - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    return i0, i1, src - i0.to(F64)


def bilinear_weights(h, w, scale):
    """(y0, y1, x0, x1, [w00, w01, w10, w11] as [OH, OW] float64) of the map h x w enlarged by 1 / scale."""
    OH, OW = int(round(h / scale)), int(round(w / scale))
    y0, y1, ly = up_coords(OH, h, scale)
    x0, x1, lx = up_coords(OW, w, scale)
    ly, lx = ly.view(-1, 1), lx.view(1, -1)
    return y0, y1, x0, x1, [(1 - ly) * (1 - lx), (1 - ly) * lx, ly * (1 - lx), ly * lx]


def bilinear_ref(a, ea, scale, extra_terms=0):
    """a [..., h, w] float64 with errors ea (a tensor or 0) -> (v, ev) [..., OH, OW]: the four-tap sum in fp32 from inputs within ea."""
    h, w = a.shape[-2:]
    y0, y1, x0, x1, W = bilinear_weights(h, w, scale)
    g = lambda t, yy, xx: t[..., yy, :][..., :, xx]
    taps = [(y0, x0), (y0, x1), (y1, x0), (y1, x1)]
    v = sum(wt * g(a, yy, xx) for wt, (yy, xx) in zip(W, taps))
    mag = sum(wt * g(a.abs(), yy, xx) for wt, (yy, xx) in zip(W, taps))
    if torch.is_tensor(ea):
        es = sum(wt * g(ea, yy, xx) for wt, (yy, xx) in zip(W, taps))
    else:
        es = torch.zeros_like(v)
    return v, es + gamma(4 + extra_terms) * (mag + es) + 5 * FTZ, mag


# ---- the exact ops --------------------------------------------------------------------------------------------------------------------
def maxpool_ref(x, relu):
    """x bf16 [B, H, W, C] -> y [B, OH, OW, C], exact."""
    x = d64(x)
    B, H, W, C = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.full((B, OH, OW, C), 0.0 if relu else -math.inf, dtype=F64)
    for dy in range(3):
        for dx in range(3):
            ih, iw = torch.arange(OH) * 2 - 1 + dy, torch.arange(OW) * 2 - 1 + dx
            oky, okx = (ih >= 0) & (ih < H), (iw >= 0) & (iw < W)
            t = x[:, ih.clamp(0, H - 1)][:, :, iw.clamp(0, W - 1)]
            t = torch.where((oky.view(-1, 1) & okx.view(1, -1)).view(1, OH, OW, 1), t, torch.full_like(t, -math.inf))
            y = torch.maximum(y, t)
    return {'y': (y, torch.zeros_like(y))}


def mask_merge_ref(inmask, pred, src, *, H, W, pl, pt, Kold, float_mode):
    src = [int(s) for s in src]
    z = torch.zeros((H, W), dtype=F64)
    if float_mode:
        m = d64(inmask)
        nf, h0, w0 = m.shape
        full = torch.zeros((nf, H, W), dtype=F64)
        full[:, pt:pt + h0, pl:pl + w0] = m
        inside = torch.zeros((H, W), dtype=torch.bool)
        inside[pt:pt + h0, pl:pl + w0] = True
        covered = torch.where(inside, full.max(0).values, z) > 0.5
    else:
        h0, w0 = inmask.shape
        ids = torch.zeros((H, W), dtype=torch.int64)
        ids[pt:pt + h0, pl:pl + w0] = inmask.detach().cpu().long()
        covered = ids > 0
    out = []
    for t, s in enumerate(src):
        if s >= 0:
            out.append(full[s] if float_mode else (ids == s).to(F64))
        elif pred is not None and t < Kold:
            out.append(torch.where(covered, z, d64(pred)[t + 1]))
        else:
            out.append(z)
    y = torch.stack(out)
    return {'planes': (y, torch.zeros_like(y))}


# ---- IMG_PREP ---------------------------------------------------------------------------------------------------------------------------
def others_ref(a, ea, k_axis=0):
    """clamp(sum_k a_k - a, 0, 1) evaluated in fp32 from values within ea of a: (y, e)."""
    K = a.shape[k_axis]
    S, Sa = a.sum(k_axis, keepdim=True), a.abs().sum(k_axis, keepdim=True)
    Se = ea.sum(k_axis, keepdim=True) if torch.is_tensor(ea) else torch.zeros_like(S)
    e = Se + ea + gamma(K + 1) * (Sa + Se + a.abs() + ea) + (K + 1) * FTZ
    y = (S - a).clamp(0, 1)
    if K == 1:
        return torch.zeros_like(y), torch.zeros_like(y)
    return y, e


def img_prep_ref(img, masks, mean, std, *, H, W, pl, pt):
    img = d64(img)
    _, h0, w0 = img.shape
    K = masks.shape[0] if masks is not None else 1
    m = torch.tensor([float(np.float32(v)) for v in mean], dtype=F64).view(3, 1, 1)
    s = torch.tensor([float(np.float32(v)) for v in std], dtype=F64).view(3, 1, 1)
    full = torch.zeros((3, H, W), dtype=F64)
    full[:, pt:pt + h0, pl:pl + w0] = img
    v = (full - m) / s
    y, b = torch.zeros((K, H, W, 8), dtype=F64), torch.zeros((K, H, W, 8), dtype=F64)
    y[..., 0:3] = v.permute(1, 2, 0)
    b[..., 0:3] = with_bf16_store(v, gamma(2) * v.abs() + 2 * FTZ).permute(1, 2, 0)
    if masks is not None:
        mk = d64(masks)
        y[..., 3] = bf16_round(mk)
        o, eo = others_ref(mk, torch.zeros_like(mk))
        y[..., 4] = o
        b[..., 4] = with_bf16_store(o, eo) if K > 1 else 0.0
    return {'y': (y, b)}


# ---- UPSAMPLE2X_ADD ---------------------------------------------------------------------------------------------------------------------
def group_of(B, skip_group):
    """The skip map of every object: (map index [B], pixels between two maps)."""
    if skip_group is None:
        return [0] * B, 0
    kg, stride = skip_group
    if isinstance(kg, int):
        return [b // kg for b in range(B)], stride
    return [c for c, k in enumerate(kg) for _ in range(k)], stride


def upsample2x_add_ref(g, skips, grp):
    """g bf16 [B, h, w, C]; skips: list of bf16 [2h, 2w, C] maps, grp[b] = the map object b adds."""
    g = d64(g).permute(0, 3, 1, 2)
    v, _, mag = bilinear_ref(g, 0, 0.5)
    sk = torch.stack([d64(skips[q]) for q in grp]).permute(0, 3, 1, 2)
    y = v + sk
    e = gamma(5) * (mag + sk.abs()) + 5 * FTZ
    return {'y': (y.permute(0, 2, 3, 1).contiguous(), with_bf16_store(y, e).permute(0, 2, 3, 1).contiguous())}


# ---- AREA_DOWN --------------------------------------------------------------------------------------------------------------------------
def area_down_ref(x, r, Cz=None):
    """x [B, H, W, C] (bf16 or f32; the C real channels) -> [B, H / r, W / r, max(C, Cz)]; channels [C, Cz) exact zeros."""
    x = d64(x)
    B, H, W, C = x.shape
    oh, ow = H // r, W // r
    t = x[:, :oh * r, :ow * r].reshape(B, oh, r, ow, r, C)
    y, ma = t.mean((2, 4)), t.abs().mean((2, 4))
    b = with_bf16_store(y, gamma(r * r + 1) * ma + (r * r + 1) * FTZ)
    if Cz is not None and Cz > C:
        z = torch.zeros((B, oh, ow, Cz - C), dtype=F64)
        y, b = torch.cat([y, z], -1), torch.cat([b, z], -1)
    return {'y': (y, b)}


# ---- MASK_DOWN --------------------------------------------------------------------------------------------------------------------------
def mask_down_ref(m, em=0, r=16):
    """m [K, H, W] float64 (within em) -> m16 [K, h, w] and pair [K, h, w, 8] = (bf16 m16, bf16 others, 0 ..)."""
    m = d64(m)
    K, H, W = m.shape
    h, w = H // r, W // r
    pool = lambda t: t.reshape(K, h, r, w, r).mean((2, 4))
    a, aa = pool(m), pool(m.abs())
    ein = pool(em) if torch.is_tensor(em) else torch.zeros_like(a)
    ea = ein + gamma(r * r) * (aa + ein) + FTZ
    y, b = torch.zeros((K, h, w, 8), dtype=F64), torch.zeros((K, h, w, 8), dtype=F64)
    y[..., 0], b[..., 0] = a, with_bf16_store(a, ea)
    o, eo = others_ref(a, ea)
    y[..., 1] = o
    b[..., 1] = with_bf16_store(o, eo) if K > 1 else 0.0
    return {'m16': (a, ea), 'pair': (y, b)}


# ---- GAP / ECA --------------------------------------------------------------------------------------------------------------------------
def gap_ref(x):
    """x bf16 [B, HW, C] -> part [B, nchunk, C] (sums of 64-pixel chunks), y [B, C] (means)."""
    x = d64(x)
    B, HW, C = x.shape
    n = -(-HW // 64)
    xp = torch.zeros((B, n * 64, C), dtype=F64)
    xp[:, :HW] = x
    part, pa = xp.view(B, n, 64, C).sum(2), xp.abs().view(B, n, 64, C).sum(2)
    y, ya = x.mean(1), x.abs().mean(1)
    return {'part': (part, gamma(64) * pa + 64 * FTZ), 'y': (y, gamma(HW + 2) * ya + (HW + 2) * FTZ)}


def eca_mean_ref(HW, part=None, fixed=None):
    if fixed is not None:
        mean = d64(fixed) / 16777216.0 / HW
        return mean, gamma(3) * mean.abs() + 3 * FTZ
    p = d64(part)
    n = p.shape[1]
    return p.sum(1) / HW, gamma(n + 2) * p.abs().sum(1) / HW + (n + 2) * FTZ


def sigmoid_fast_err(a, ea):
    return ea / 4 + (a.abs() / 4 + 4) * U32 + FTZ


def eca_apply_ref(x, r, wk, *, part=None, fixed=None):
    """x, r bf16 [B, HW, C]; wk f32 [5]; part f32 [B, nchunk, C] or fixed int64 [B, C] -> gap_out [B, C], y [B, HW, C] and (key 'pre') y
    with its bound BEFORE the bf16 store, for the head."""
    x, r, wk = d64(x), d64(r), d64(wk)
    B, HW, C = x.shape
    mean, em = eca_mean_ref(HW, part, fixed)
    pad = lambda t: torch.nn.functional.pad(t, (2, 2))
    mp, mpa, ep = pad(mean), pad(mean.abs()), pad(em)
    a = sum(wk[j] * mp[:, j:j + C] for j in range(5))
    ea = sum(wk[j].abs() * ep[:, j:j + C] for j in range(5)) + gamma(5) * sum(wk[j].abs() * (mpa[:, j:j + C] + ep[:, j:j + C]) for j in range(5)) + 5 * FTZ
    s = torch.sigmoid(a)
    es = sigmoid_fast_err(a, ea)
    y = x * s[:, None] + r
    e = x.abs() * es[:, None] + gamma(2) * (x.abs() * (s + es)[:, None] + r.abs()) + 2 * FTZ
    return {'gap_out': (mean, em), 'y': (y, with_bf16_store(y, e)), 'pre': (y, e)}


def eca_head_ref(w, bias, *, pre=None, stored=None):
    """plog [B, HW] = bias + sum_c relu(y_stored[.., c]) w[c]: from the reference's y before the store (pre = (y64, e): the stored value lies
    in [bf16(y64 - e), bf16(y64 + e)]) or from the stored y itself."""
    w = d64(w).view(1, 1, -1)
    if stored is not None:
        lo = hi = d64(stored)
    else:
        lo, hi = bf16_round(pre[0] - pre[1]), bf16_round(pre[0] + pre[1])
    t0, t1 = lo.clamp(min=0) * w, hi.clamp(min=0) * w
    L, Uu = torch.minimum(t0, t1).sum(-1), torch.maximum(t0, t1).sum(-1)
    mag = torch.maximum(t0.abs(), t1.abs()).sum(-1)
    bv = float(d64(bias).view(-1)[0]) if bias is not None else 0.0
    return {'plog': ((L + Uu) / 2 + bv, (Uu - L) / 2 + gamma(514) * (mag + abs(bv)) + 514 * FTZ)}


# ---- GRU --------------------------------------------------------------------------------------------------------------------------------
def gru_ref(values, h):
    """values f32 [n, 3C], h f32 [n, C] (the state BEFORE the launch) -> h [n, C] (fp32) and hb (its bf16 shadow)."""
    v, h = d64(values), d64(h)
    C = h.shape[1]
    a, b, c = v[:, :C], v[:, C:2 * C], v[:, 2 * C:]
    f, u, n = torch.sigmoid(a), torch.sigmoid(b), torch.tanh(c)
    ef, eu = sigmoid_fast_err(a, 0), sigmoid_fast_err(b, 0)
    en = TANH_ULP * 2 * U32 * n.abs() + FTZ
    q = torch.sigmoid(-b)                                                  # 1 - u without the cancellation
    y = f * h * q + u * n
    ha = h.abs()
    e = ha * (q + eu) * ef + ha * (f + ef) * eu + gamma(4) * ha * (f + ef) * (q + eu) \
        + (n.abs() + en) * eu + u * en + gamma(2) * ((u + eu) * (n.abs() + en) + ha * (f + ef) * (q + eu)) + 6 * FTZ
    return {'h': (y, e), 'hb': (y, with_bf16_store(y, e))}


# ---- the seg tail -----------------------------------------------------------------------------------------------------------------------
def logit64(q):
    return torch.log(q / (1 - q))


def clamp_logit_ref(p, ep, one_minus=None):
    """(y, e) of clamp_logit evaluated in fp32 on an input within ep of p (float64)."""
    ep = ep if torch.is_tensor(ep) else torch.full_like(p, float(ep))
    c, lo, hi = p.clamp(LO32, HI32), (p - ep).clamp(LO32, HI32), (p + ep).clamp(LO32, HI32)
    y, yl, yh = logit64(c), logit64(lo), logit64(hi)
    e_ratio = -math.log1p(-(2 * U32 + 3 * U32 * U32))
    big = torch.maximum(yl.abs(), yh.abs()) + e_ratio
    e1 = e_ratio + LOG_ULP * 2 * U32 * big + 4 * U64 / (1 - hi) + FTZ
    return y, torch.maximum(yh - y, y - yl) + e1


def prob_bg_ref(q, eq):
    """bg = prod_k q_k, multiplied up in object order in fp32 from factors q'_k <= 1 within eq of q [K, ...]: (bg, e).  A step r <- fl(r q'_k)
    carries the error so far through the factor and rounds once; the rounding is at most u of the product and, r and q'_k being fp32 numbers no
    smaller than the product, at most 1 - q'_k and at most 1 - r: next to 1 a product moves by what its factors lack, not by u."""
    r, e = torch.ones_like(q[0]), torch.zeros_like(q[0])
    for k in range(q.shape[0]):
        up = (r + e) * (q[k] + eq[k])
        rnd = torch.minimum(U32 * up, torch.minimum(1 - q[k] + eq[k], 1 - r + e)) + 2 * U64
        r, e = r * q[k], up - r * q[k] + rnd
    return r, e + FTZ


def one_minus_err(p, ep):
    """The error of fl(1 - p') against 1 - p for p' within ep of p in [0, 1]: exact for p' >= 1/2 (Sterbenz); else one rounding, which is at most
    u of the result and at most p' itself (1 is an fp32 number)."""
    return ep + torch.where(p < 0.5, torch.minimum(U32 * (1 - p + ep), p + ep), torch.zeros_like(p))


def sigmoid_exact_err(x):
    """p = 1 / (1 + expf(-x)) and q = 1 - p in float64 with the error of the fp32 p.  E = e^-x carries 4 u relative (p q 4 u of p); s = fl(1 + E)
    is off by at most min(u s, E, 1) -- both 1 and E are fp32 numbers, and rounding to nearest never lands farther than either -- a relative
    min(u, q, p) of p; the division 1 / s is one rounding, and none at all where s == 1 exactly (E below half an ulp of 1, 2^-24)."""
    E = torch.exp(-x)
    p, q = 1 / (1 + E), torch.where(torch.isinf(E), torch.ones_like(E), E / (1 + E))
    d_add = torch.minimum(torch.minimum(q, p), torch.full_like(p, U32))
    d_div = torch.where(E * (1 + 8 * U32) < 2.0 ** -24, torch.zeros_like(p), torch.full_like(p, U32))
    return p, q, p * (4 * U32 * q + d_add + d_div) * (1 + 1e-6) + FTZ


def agg_ref(x):
    """SEG_AGG: raw logits x [K, ...] -> aggregated, clamped logits [K + 1, ...] (plane 0 = background) with their bounds."""
    p, q, ep = sigmoid_exact_err(d64(x))
    eq = one_minus_err(p, ep)
    bg, ebg = prob_bg_ref(q, eq)
    l0, e0 = clamp_logit_ref(bg, ebg)
    lk, ek = clamp_logit_ref(p, ep)
    return torch.cat([l0[None], lk]), torch.cat([e0[None], ek])


def seg_agg_ref(x):
    y, e = agg_ref(x)
    return {'agg': (y, e)}


def softmax_ref(v, ev):
    """Softmax over dim 0 of logits within ev of v, evaluated in fp32: (w, bound).  With t_j the logits' errors,
    w'_c = 1 / (1 + sum_{j != c} e^((v_j + t_j) - (v_c + t_c))) lies between the two values at t_j - t_c = +-(e_j + e_c): a plane that
    dominates its pixel moves by the others' weights times their errors, not by its own error."""
    P = v.shape[0]
    mx = v.max(0, keepdim=True).values
    ex = torch.exp(v - mx)
    w = ex / ex.sum(0, keepdim=True)
    lo, hi = torch.empty_like(w), torch.empty_like(w)
    for c in range(P):
        d = v - v[c:c + 1]
        up, dn = torch.exp(d + ev + ev[c:c + 1]), torch.exp(d - ev - ev[c:c + 1])
        up[c], dn[c] = 0.0, 0.0
        lo[c], hi[c] = 1 / (1 + up.sum(0)), 1 / (1 + dn.sum(0))
    Em = ev.max(0, keepdim=True).values
    a = (((v - mx).abs() + ev + Em) * (1 + U32) + 4) * U32
    b = a.max(0, keepdim=True).values + gamma(P)
    rel = (1 + a) * (1 + U32) ** 2 / (1 - b) - 1
    return w, torch.maximum(hi - w, w - lo) + hi * rel + 8 * U64 + 2 * FTZ


def up4_softmax_ref(agg, eagg=0):
    """agg [P, h, w] (aggregated logits, exact inputs or within eagg) -> logits_up, prob [P, 4h, 4w]."""
    v, ev, _ = bilinear_ref(d64(agg), eagg, 0.25)
    w, ew = softmax_ref(v, ev)
    return {'lup': (v, ev), 'prob': (w, ew)}


def up4_fused_ref(x, mask_down=False):
    """The fused forms, from the raw logits x [K, h, w]; with the mask-down outputs when asked."""
    a, ea = agg_ref(x)
    out = up4_softmax_ref(a, ea)
    if mask_down:
        w, ew = out['prob']
        out.update(mask_down_ref(w[1:], ew[1:]))
    return out


def agg_softmax_ref(planes):
    p = d64(planes)
    q = 1 - p
    bg, ebg = prob_bg_ref(q, one_minus_err(p, torch.zeros_like(p)))
    l0, e0 = clamp_logit_ref(bg, ebg)
    lk, ek = clamp_logit_ref(p, 0.0)
    w, ew = softmax_ref(torch.cat([l0[None], lk]), torch.cat([e0[None], ek]))
    return {'prob': (w, ew)}


# =========================================================================================================================================
# Inputs: the regimes shared per op
# =========================================================================================================================================
def gen(seed):
    return torch.Generator().manual_seed(seed)


def bf16_map(g, shape, regime):
    """'plain' randn / 2; 'large' the same x 2^6; 'sparse' mostly exact zeros with per-channel scales 2^-6 .. 2^6."""
    v = torch.randn(shape, generator=g)
    if regime == 'plain':
        v = v * 0.5
    elif regime == 'large':
        v = v * 32.0
    elif regime == 'sparse':
        v = (v - 0.45).clamp(min=0) * torch.exp2(torch.rand(shape[-1], generator=g) * 12 - 6)
    elif regime == 'negative':
        v = -v.abs() - 0.25
    else:
        raise ValueError(regime)
    return v.to(BF16)


def seg_logits(g, K, h, w, regime):
    """'plain' randn x 3; 'large' +-25 plateaus joined by ramps through 0, every object with its own period and phase (with one object
    saturated and the others anywhere: every plane on a clamp, one object at 1, the background at 0, and the transitions between them)."""
    if regime == 'plain':
        return torch.randn((K, h, w), generator=g) * 3
    t = (torch.arange(h * w, dtype=F32) + torch.rand(1, generator=g)) / max(h * w, 1)
    k = torch.arange(K, dtype=F32).view(K, 1)
    s = ((t.view(1, -1) * (k + 1) + k / 3 + 0.21) % 1) * 2 - 1
    x = 25 * (2.5 * s).clamp(-1, 1) + torch.randn((K, h * w), generator=g) * 0.05
    return x.view(K, h, w).contiguous()


def soft_masks(g, K, H, W, regime):
    """'plain' uniform in [0, 1] (sums above 1 for K >= 2); 'hard' exactly 0 / 1: a one-hot of K + 1 labels per pixel, with one corner where two
    objects overlap (sum 2)."""
    if regime == 'plain':
        return torch.rand((K, H, W), generator=g)
    lab = torch.randint(0, K + 1, (H, W), generator=g)
    m = torch.stack([(lab == k + 1).float() for k in range(K)])
    if K > 1:
        m[:2, :max(1, H // 4), :max(1, W // 4)] = 1.0
    return m


def gru_inputs(g, n, C, regime):
    v = torch.randn((n, 3 * C), generator=g) * 2
    h = torch.randn((n, C), generator=g)
    if regime == 'large':
        v = torch.where(torch.rand((n, 3 * C), generator=g) < 0.7, torch.sign(v) * 90.0, v * 8)
        h = h * 16
    return v, h


# =========================================================================================================================================
# The shared cases.  Every runner builds its buffers on `dev` between guards (outputs pre-filled with NaN), hands the launch list to
# `launch(ol)` -- the HIP executor or the interpreter; it returns a callable that runs the same launches again -- and asserts: every element
# within its bound, every exact property, the guards intact, a second run bit-identical, and the promised bit-identities between forms.
# `mutate(ctx)`, used by test_px_ref64_cpu.py, overwrites outputs between the launch and the checks.  Each returns {label: worst ratio}.
# =========================================================================================================================================
def finish(b, again, ratios, rerun=True):
    assert b.guards_intact(), 'a guard element was overwritten'
    if rerun and again is not None:
        first = b.snapshot()
        b.reset()
        again()
        for n, t in first.items():
            assert torch.equal(bits(b[n]), bits(t)), (n, 'a second run of the same launches differs')
        assert b.guards_intact()
    return ratios


def same_bits(a, c, what):
    assert torch.equal(bits(a), bits(c)), (what, 'forms that are promised to be bit-identical differ', int((bits(a) != bits(c)).sum()))


def out_nan(b, name, shape, dtype=F32):
    return b.output(name, shape, dtype, NAN)


def sentinel_filled(b, name, shape, dtype=BF16):
    """An output whose gaps must survive: pre-filled with the sentinel, not NaN."""
    return b.output(name, shape, dtype)


# ---- MAXPOOL / IMG_PREP -----------------------------------------------------------------------------------------------------------------
MAXPOOL_CASES = [dict(H=H, W=W, C=C, relu=relu, regime=rg) for (H, W) in ((1, 1), (7, 9), (8, 8)) for C in (8, 64) for relu in (False, True)
                 for rg in ('plain', 'negative')]


def run_maxpool(dev, launch, *, H, W, C, relu, regime, B=2, mutate=None):
    g = gen(H * 100 + W + C)
    x = bf16_map(g, (B, H, W, C), regime)
    b = Bufs(dev)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = out_nan(b, 'y', (B, OH, OW, C), BF16)
    ol = O.OpList()
    ol.maxpool(b.operand(x), y, B=B, H=H, W=W, C=C, relu=relu)
    again = launch(ol)
    if mutate:
        mutate(SimpleNamespace(x=x, y=y, relu=relu))
    ref = maxpool_ref(x, relu)
    assert all_finite(ref)
    r = chk(y, ref['y'], 'maxpool')
    if regime == 'negative':
        assert bool((y.float() == 0).all()) if relu else bool((y.float() < 0).all())
    return finish(b, None if mutate else again, {'y': r})


IMG_PREP_CASES = [dict(K=K, regime=rg) for K in (0, 1, 3) for rg in ('plain', 'hard') if K or rg == 'plain']
IMG_MEAN, IMG_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def run_img_prep(dev, launch, *, K, regime, mutate=None):
    h0, w0, H, W, pl, pt = 30, 43, 32, 48, 2, 1
    g = gen(K * 7 + len(regime))
    img = torch.rand((3, h0, w0), generator=g)
    masks = soft_masks(g, K, H, W, regime) if K else None
    b = Bufs(dev)
    y = out_nan(b, 'y', (max(K, 1), H, W, 8), BF16)
    ol = O.OpList()
    ol.img_prep(b.operand(img), b.operand(masks) if K else None, y, h0=h0, w0=w0, H=H, W=W, pad_left=pl, pad_top=pt, K=K, mean=IMG_MEAN, std=IMG_STD)
    again = launch(ol)
    if mutate:
        mutate(SimpleNamespace(img=img, masks=masks, y=y, K=K))
    ref = img_prep_ref(img, masks, IMG_MEAN, IMG_STD, H=H, W=W, pl=pl, pt=pt)
    assert all_finite(ref)
    r = chk(y, ref['y'], 'img_prep')
    assert bool((y[..., 5:].float() == 0).all())
    return finish(b, None if mutate else again, {'y': r})


# ---- UPSAMPLE2X_ADD ---------------------------------------------------------------------------------------------------------------------
UPSAMPLE_CASES = [dict(h=h, w=w, C=C, B=3, group=None, regime=rg) for (h, w) in ((1, 1), (1, 5), (3, 1), (7, 9)) for C in (8, 128)
                  for rg in (('plain', 'large', 'sparse') if (h, w) == (7, 9) else ('plain',))] + \
                 [dict(h=3, w=5, C=8, B=4, group=(2, 'stride'), regime='plain'), dict(h=7, w=9, C=128, B=4, group=(2, 'stride'), regime='sparse'),
                  dict(h=3, w=5, C=8, B=4, group=((1, 3), 'stride'), regime='plain'), dict(h=7, w=9, C=128, B=5, group=((2, 1, 2), 'stride'), regime='plain')]


def run_upsample(dev, launch, *, h, w, C, B, group, regime, mutate=None):
    g = gen(h * 31 + w + C + B)
    x = bf16_map(g, (B, h, w, C), regime)
    nmap = 1 if group is None else (B // group[0] if isinstance(group[0], int) else len(group[0]))
    stride = 4 * h * w + 3                                                  # pixels between two skip maps: more than one map
    skip = bf16_map(g, (nmap, stride, C), regime)
    skip[:, 4 * h * w:] = NAN                                               # the pixels between the maps are never read
    b = Bufs(dev)
    dx, dsk = b.operand(x), b.operand(skip)
    y = out_nan(b, 'y', (B, 2 * h, 2 * w, C), BF16)
    sg = None if group is None else (group[0], stride)
    grp, _ = group_of(B, sg)
    ol = O.OpList()
    ol.upsample2x_add(dx, dsk, y, B=B, h=h, w=w, C=C, skip_group=sg)
    y1 = None
    if group is not None:                                                   # the grouped launch = one launch per object with its group's map
        y1 = out_nan(b, 'y1', (B, 2 * h, 2 * w, C), BF16)
        for o in range(B):
            ol.upsample2x_add(dx[o:], dsk[grp[o]], y1[o:], B=1, h=h, w=w, C=C)
    again = launch(ol)
    if mutate:
        mutate(SimpleNamespace(x=x, skip=skip, ys=[y] + ([y1] if y1 is not None else []), grp=grp, h=h, w=w))
    ref = upsample2x_add_ref(x, [skip[q, :4 * h * w].view(2 * h, 2 * w, C) for q in range(nmap)], grp)
    assert all_finite(ref)
    r = {'y': chk(y, ref['y'], 'upsample2x_add')}
    if y1 is not None:
        same_bits(y, y1, 'upsample2x_add groups against one launch per object')
    return finish(b, None if mutate else again, r)


# ---- AREA_DOWN / AREA_DOWN3 -------------------------------------------------------------------------------------------------------------
AREA_CASES = [dict(r=r, C=C, regime=rg) for r in (2, 3, 4, 8) for C in (8, 128) for rg in (('plain', 'large', 'sparse') if C == 128 and r in (2, 4) else ('plain',))]


def run_area(dev, launch, *, r, C, regime, mutate=None):
    """One AREA_DOWN3 launch over three segments -- a bf16 slice of a wider buffer into a slice of a concat buffer, a second bf16 map, an f32
    map with C = 1 and Cz = 8 -- against three AREA_DOWN launches (same bits), the run-time-r form (same bits), and float64."""
    B, oh, ow = 2, 3, 5
    H, W = oh * r + (1 if r == 3 else 0), ow * r
    oh, ow = H // r, W // r
    g = gen(r * 10 + C)
    ldx, CT = C + 8, 2 * C + 16
    xa = torch.full((B, H, W, ldx), NAN, dtype=BF16)
    xa[..., :C] = bf16_map(g, (B, H, W, C), regime)
    xb = bf16_map(g, (B, H, W, C), regime)
    xf = seg_logits(g, B, H, W, 'plain').view(B, H, W, 1).contiguous()
    b = Bufs(dev)
    da, db, df = b.operand(xa), b.operand(xb), b.operand(xf)
    cats = {n: sentinel_filled(b, n, (B, oh, ow, CT)) for n in ('cat3', 'cat1', 'cat3rt')}
    segs = lambda cat: [dict(x=da, y=cat, B=B, H=H, W=W, C=C, ldx=ldx, ldy=CT, r=r),
                        dict(x=db, y=cat.view(-1)[C:], B=B, H=H, W=W, C=C, ldx=C, ldy=CT, r=r),
                        dict(x=df, y=cat.view(-1)[2 * C:], B=B, H=H, W=W, C=1, ldx=1, ldy=CT, r=r, f32_in=True, Cz=8)]
    ol = O.OpList()
    k3 = ol.area_down3(segs(cats['cat3']))
    for s in segs(cats['cat1']):
        ol.area_down(s['x'], s['y'], B=B, H=H, W=W, C=s['C'], ldx=s['ldx'], ldy=CT, r=r, f32_in=s.get('f32_in', False), Cz=s.get('Cz'))
    krt = ol.area_down3(segs(cats['cat3rt']))
    kind, fl, *rest = ol.recs[k3]
    ol.recs[k3] = (kind, fl & ~8, *rest)
    kind, fl, *rest = ol.recs[krt]
    ol.recs[krt] = (kind, fl | 8, *rest)
    again = launch(ol)
    if mutate:
        mutate(SimpleNamespace(xa=xa, xb=xb, xf=xf, cats=cats, C=C, r=r))
    refs = [area_down_ref(xa[..., :C], r), area_down_ref(xb, r), area_down_ref(xf, r, Cz=8)]
    ratios = {}
    for n, cat in cats.items():
        c = cat.cpu()
        for q, (ref, c0, cn) in enumerate(zip(refs, (0, C, 2 * C), (C, C, 8))):
            assert all_finite(ref)
            ratios[f'{n}.{q}'] = chk(c[..., c0:c0 + cn], ref['y'], f'area_down {n} segment {q}')
        assert bool((c[..., 2 * C + 1:2 * C + 8].float() == 0).all()) and bool((c[..., 2 * C + 8:] == SENT_F).all()), 'zero fill / the gap behind it'
    same_bits(cats['cat3'], cats['cat1'], 'AREA_DOWN3 against three AREA_DOWNs')
    same_bits(cats['cat3'], cats['cat3rt'], 'compile-time r against run-time r')
    return finish(b, None if mutate else again, ratios)


# ---- MASK_DOWN --------------------------------------------------------------------------------------------------------------------------
MASK_DOWN_CASES = [dict(K=K, H=H, W=W, pitch=p, regime=rg) for K in (1, 4, 5) for (H, W) in ((16, 16), (32, 48)) for p in (8, 64) for rg in ('plain', 'hard')]


def check_mask_down(m16, pair, ref, pitch, what):
    r = {'m16': chk(m16, ref['m16'], what + ' m16'), 'pair': chk(pair[..., :8], ref['pair'], what + ' pair')}
    assert bool((pair[..., 2:8].float() == 0).all()), 'channels 2 .. 7 are zeros'
    if pitch > 8:
        assert bool((pair[..., 8:] == SENT_F).all()), 'channels 8 .. of a 64-pitch pair were written'
    return r


def run_mask_down(dev, launch, *, K, H, W, pitch, regime, mutate=None):
    g = gen(K + H + W + pitch)
    m = soft_masks(g, K, H, W, regime)
    b = Bufs(dev)
    h, w = H // 16, W // 16
    m16, pair = out_nan(b, 'm16', (K, h, w)), sentinel_filled(b, 'pair', (K, h, w, pitch))
    ol = O.OpList()
    ol.mask_down(b.operand(m), pair, m16, K=K, H=H, W=W, pair_channels=pitch)
    again = launch(ol)
    if mutate:
        mutate(SimpleNamespace(m=m, m16=m16, pair=pair, K=K))
    ref = mask_down_ref(m)
    assert all_finite(ref)
    r = check_mask_down(m16, pair, ref, pitch, 'mask_down')
    if K == 1:
        assert bool((pair[..., 1].float() == 0).all())
    return finish(b, None if mutate else again, r)


# ---- GAP / ECA_APPLY --------------------------------------------------------------------------------------------------------------------
GAP_HW = (1, 31, 32, 33, 63, 64, 65, 513)
GAP_CASES = [dict(HW=HW, C=C, regime=rg) for HW in GAP_HW for C in (8, 32, 64, 128, 256)
             for rg in (('plain', 'large', 'sparse') if (HW, C) in ((513, 256), (65, 64)) else ('plain',))]


def run_gap_eca(dev, launch, *, HW, C, regime, mutate=None):
    """GAP (with and without partial_only) and ECA_APPLY from the partials and from fixed sums, with and without gap_out; at C = 256 each with
    the fused head (bias present and absent)."""
    B = 2
    g = gen(HW * 3 + C)
    x, res = bf16_map(g, (B, HW, C), regime), bf16_map(g, (B, HW, C), regime)
    wk = torch.randn(5, generator=g) * 0.7
    pw, pb = (torch.randn(256, generator=g) / 8).to(BF16), torch.randn(1, generator=g)
    fixed = (gap_fixed(x.float()).sum(1) * 16).to(I64)
    n = -(-HW // 64)
    b = Bufs(dev)
    dx, dr, dwk, dfx = b.operand(x), b.operand(res), b.operand(wk), b.operand(fixed)
    head_w = lambda bias: SimpleNamespace(cout=1, kh=1, cin_padded=256, weight=b.operand(pw), bias=b.operand(pb) if bias else None)
    part, part2, gy = out_nan(b, 'part', (B, n, C)), out_nan(b, 'part2', (B, n, C)), out_nan(b, 'gy', (B, C))
    ol = O.OpList()
    ol.gap(dx, gy, B=B, HW=HW, C=C, scratch=part2)
    ol.gap(dx, None, B=B, HW=HW, C=C, scratch=part, partial_only=True)
    forms = {}
    for src in ('part', 'fixed'):
        for go in (True, False):
            for head in ((None, 'bias', 'nobias') if C == 256 else (None,)):
                if head and not go:
                    continue
                name = f'{src}{"+gap" if go else ""}{"+" + head if head else ""}'
                y = out_nan(b, 'y_' + name, (B, HW, C), BF16)
                gout = out_nan(b, 'g_' + name, (B, C)) if go else None
                plog = out_nan(b, 'p_' + name, (B, HW)) if head else None
                kw = dict(fixed_sums=dfx) if src == 'fixed' else dict(part=part)
                ol.eca_apply(dx, gout, dwk, dr, y, B=B, HW=HW, C=C, head=(head_w(head == 'bias'), plog) if head else None, **kw)
                forms[name] = (src, y, gout, plog, head)
    again = launch(ol)
    if mutate:
        mutate(SimpleNamespace(x=x, res=res, wk=wk, pw=pw, pb=pb, part=part, gy=gy, forms=forms, HW=HW, C=C, B=B))
    gref = gap_ref(x)
    assert all_finite(gref)
    r = {'gap.part': chk(part, gref['part'], 'gap partials'), 'gap.y': chk(gy, gref['y'], 'gap mean')}
    same_bits(part, part2, 'the partials with and without partial_only')
    for name, (src, y, gout, plog, head) in forms.items():
        ref = eca_apply_ref(x, res, wk, part=part, fixed=None) if src == 'part' else eca_apply_ref(x, res, wk, fixed=fixed)
        assert all_finite(ref)
        r[name + '.y'] = chk(y, ref['y'], 'eca ' + name)
        if gout is not None:
            r[name + '.gap'] = chk(gout, ref['gap_out'], 'eca gap_out ' + name)
        if head:
            bias = pb if head == 'bias' else None
            hull, tight = eca_head_ref(pw, bias, pre=ref['pre']), eca_head_ref(pw, bias, stored=y)
            assert all_finite(hull) and all_finite(tight)
            r[name + '.head'] = chk(plog, hull['plog'], 'eca head (hull) ' + name)
            r[name + '.head_stored'] = chk(plog, tight['plog'], 'eca head (from the stored y) ' + name)
        same_bits(y, forms[src][1], 'eca y with and without gap_out / head')
    return finish(b, None if mutate else again, r)


# ---- GRU --------------------------------------------------------------------------------------------------------------------------------
GRU_CASES = [dict(n=n, C=C, regime=rg) for (n, C) in ((1, 4), (3, 64), (5, 256), (257, 8), (7, 6)) for rg in ('plain', 'large')]


def run_gru(dev, launch, *, n, C, regime, mutate=None):
    """gru4 (the default), the scalar kernel through GRU_SCALAR, and the scalar fallback through an hb offset by 2 bytes: the same bits."""
    g = gen(n + C)
    v, h0 = gru_inputs(g, n, C, regime)
    b = Bufs(dev)
    dv = b.operand(v)
    outs = {}
    ol = O.OpList()
    for form in ('default', 'scalar', 'hb+2'):
        h = b.output('h_' + form, (n, C), F32, h0)
        hb = out_nan(b, 'hb_' + form, (n * C + 1,), BF16)
        hbv = hb[1:] if form == 'hb+2' else hb[:n * C]
        k = ol.gru(dv, h, hbv, n=n, C=C)
        kind, fl, *rest = ol.recs[k]
        ol.recs[k] = (kind, (fl & ~1) | (1 if form == 'scalar' else 0), *rest)
        outs[form] = (h, hbv)
    again = launch(ol)
    if mutate:
        mutate(SimpleNamespace(v=v, h0=h0, outs=outs, C=C))
    ref = gru_ref(v, h0)
    assert all_finite(ref)
    r = {}
    for form, (h, hb) in outs.items():
        assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(hb.float()).all()), 'NaN / inf out of finite input'
        r[form + '.h'] = chk(h, ref['h'], 'gru h ' + form)
        r[form + '.hb'] = chk(hb.view(n, C), ref['hb'], 'gru hb ' + form)
        same_bits(h, outs['default'][0], 'gru forms')
        same_bits(hb, outs['default'][1], 'gru forms (bf16 shadow)')
    return finish(b, None if mutate else again, r)


# ---- SEG_AGG + UP4_SOFTMAX --------------------------------------------------------------------------------------------------------------
UP4_SIZES = ((1, 1), (1, 9), (7, 1), (2, 2), (3, 5), (5, 3), (4, 4), (4, 8), (8, 4), (8, 12), (12, 20))
UP4_CASES = [dict(K=K, h=h, w=w, regime=rg) for K in (1, 2, 3, 4, 5, 6, 7) for (h, w) in UP4_SIZES for rg in ('plain', 'large')
             if rg == 'plain' or (h, w) in ((1, 1), (3, 5), (4, 4), (8, 12), (12, 20))] + \
            [dict(K=K, h=h, w=w, regime=rg) for K in (8, 15) for (h, w) in ((1, 1), (3, 5), (8, 12)) for rg in ('plain', 'large')]
UP4_F = dict(f4=1, f4rt=1 | 8, f1=1 | 2, md=1 | 4, md_lanes=1 | 4 | 16, md_rt=1 | 4 | 8, md_rt_lanes=1 | 4 | 8 | 16)


def run_up4(dev, launch, *, K, h, w, regime, mutate=None):
    """Every form of UP4_SOFTMAX on one map of raw logits: the two-launch form (SEG_AGG + the plain kernel), the fused four-pixel kernels with the
    compile-time and the run-time object count, the one-pixel kernel (flag 2; outputs offset by 4 bytes; P > 8), logits_up = None, and at
    multiples of 4 the mask-down kernels (SH on / off, KC / run-time K) with a separate MASK_DOWN on the stored probabilities."""
    P, H, W = K + 1, 4 * h, 4 * w
    g = gen(K * 1000 + h * 30 + w + len(regime))
    x = seg_logits(g, K, h, w, regime)
    b = Bufs(dev)
    dxl = b.operand(x)
    md_ok = P <= 8 and h % 4 == 0 and w % 4 == 0
    names = ['f1'] if P > 8 else ['f4', 'f4rt', 'f1', 'off4', 'nolup'] + (['md', 'md_lanes', 'md_rt', 'md_rt_lanes'] if md_ok else [])
    outs = {}
    ol = O.OpList()
    agg = out_nan(b, 'agg', (P, h, w))
    ol.seg_agg(dxl, agg, K=K, hw=h * w)
    two_p, two_l = out_nan(b, 'two_prob', (P, H, W)), out_nan(b, 'two_lup', (P, H, W))
    ol.up4_softmax(agg, two_p, two_l, P=P, h=h, w=w)
    for n in names:
        off = 1 if n == 'off4' else 0
        prob = out_nan(b, n + '_prob', (P * H * W + off,))[off:].view(P, H, W)
        lup = None if n == 'nolup' else out_nan(b, n + '_lup', (P * H * W + off,))[off:].view(P, H, W)
        fl = UP4_F.get(n, 1)
        ptrs = [dxl, prob, lup]
        pitch = 0
        if fl & 4:
            pitch = 64 if n in ('md', 'md_rt') else 8
            m16, pair = out_nan(b, n + '_m16', (K, h // 4, w // 4)), sentinel_filled(b, n + '_pair', (K, h // 4, w // 4, pitch))
            ptrs += [m16, pair]
        ol.add(O.UP4_SOFTMAX, fl, [P, h, w, pitch, 1], [], ptrs)
        outs[n] = (prob, lup, (m16, pair, pitch) if fl & 4 else None)
    if md_ok:
        sm16, spair = out_nan(b, 'sep_m16', (K, h // 4, w // 4)), sentinel_filled(b, 'sep_pair', (K, h // 4, w // 4, 64))
        ol.mask_down(outs['f4'][0][1:], spair, sm16, K=K, H=H, W=W, pair_channels=64)
    again = launch(ol)
    if mutate:
        mutate(SimpleNamespace(x=x, agg=agg, two_p=two_p, two_l=two_l, outs=outs, K=K, h=h, w=w, sep=(sm16, spair) if md_ok else None))
    r = {}
    sref = seg_agg_ref(x)
    assert all_finite(sref)
    r['seg_agg'] = chk(agg, sref['agg'], 'seg_agg')
    pref = up4_softmax_ref(agg)                                            # the plain kernel from the aggregated logits IT read: tight
    assert all_finite(pref)
    r['plain.prob'], r['plain.lup'] = chk(two_p, pref['prob'], 'up4 plain prob'), chk(two_l, pref['lup'], 'up4 plain lup')
    fref = up4_fused_ref(x, mask_down=md_ok)
    assert all_finite(fref)
    for n, (prob, lup, md) in outs.items():
        r[n + '.prob'] = chk(prob, fref['prob'], f'up4 {n} prob')
        same_bits(prob, two_p, f'up4 {n} against the two-launch form (prob)')
        if lup is not None:
            r[n + '.lup'] = chk(lup, fref['lup'], f'up4 {n} lup')
            same_bits(lup, two_l, f'up4 {n} against the two-launch form (logits_up)')
        if md:
            m16, pair, pitch = md
            r.update({f'{n}.{k}': v for k, v in check_mask_down(m16, pair, fref, pitch, f'up4 {n}').items()})
            tight = mask_down_ref(prob[1:])
            r.update({f'{n}.{k}_stored': v for k, v in check_mask_down(m16, pair, tight, pitch, f'up4 {n} from the stored prob').items()})
            same_bits(m16, sm16, f'up4 {n} m16 against a separate MASK_DOWN')
            same_bits(pair[..., :8], spair[..., :8], f'up4 {n} pair against a separate MASK_DOWN')
    return finish(b, None if mutate else again, r)


PLAIN_HW = (1, 255, 256, 257)
PLAIN_CASES = [dict(K=K, hw=hw, regime=rg) for hw in PLAIN_HW for K in (1, 3) for rg in ('plain', 'large')]


def run_seg_plain(dev, launch, *, K, hw, regime, mutate=None):
    """SEG_AGG and the plain UP4_SOFTMAX on a one-row map of hw pixels (block boundaries of both kernels)."""
    P = K + 1
    g = gen(K * 7 + hw)
    x = seg_logits(g, K, 1, hw, regime)
    b = Bufs(dev)
    agg, prob, lup = out_nan(b, 'agg', (P, 1, hw)), out_nan(b, 'prob', (P, 4, 4 * hw)), out_nan(b, 'lup', (P, 4, 4 * hw))
    ol = O.OpList()
    ol.seg_agg(b.operand(x), agg, K=K, hw=hw)
    ol.up4_softmax(agg, prob, lup, P=P, h=1, w=hw)
    again = launch(ol)
    sref, pref, fref = seg_agg_ref(x), up4_softmax_ref(agg), up4_fused_ref(x)
    assert all_finite(sref) and all_finite(pref) and all_finite(fref)
    r = {'seg_agg': chk(agg, sref['agg'], 'seg_agg'), 'prob': chk(prob, pref['prob'], 'plain prob'), 'lup': chk(lup, pref['lup'], 'plain lup'),
         'prob_from_logits': chk(prob, fref['prob'], 'plain prob from the raw logits')}
    return finish(b, None if mutate else again, r)


CLIP_CASES = [dict(counts=c, h=h, w=w, md=md, regime=rg) for c in ((2, 2), (3, 3, 3), (1, 3), (3, 1), (7, 1, 2), (2, 2, 2))
              for (h, w, md) in ((3, 5, False), (4, 8, False), (8, 12, True), (4, 4, True)) for rg in (('plain', 'large') if (h, w) == (8, 12) else ('plain',))
              if (h, w) != (3, 5) or c in ((2, 2), (3, 3, 3))]            # (ops.up4_softmax takes the mixed form at multiples of 4 only)


def run_up4_clips(dev, launch, *, counts, h, w, md, regime, mutate=None):
    """Clips in lock step: (2, 2) and (3, 3, 3) run the uniform form (i4), the others the mixed form (i5); (2, 2, 2) as a MIXED launch too.
    The descriptors are built with their flags spelled out (the A/B constants of `ops` play no part): the shared-aggregation form, with
    mask-down also the per-lane form (flags&16: md<8, KC, false> / md_mixed<8, false>), for uniform clips also the run-time object count
    (flags&8), and one launch per clip.  Every form against float64, and all of them bit for bit against the one-clip launches."""
    uniform = counts in ((2, 2), (3, 3, 3))
    st, H, W = O.clip_starts(counts), 4 * h, 4 * w
    nobj, ncell, G = st[-1], (h // 4) * (w // 4), len(counts)
    g = gen(sum(counts) * 100 + h + w)
    x = torch.cat([seg_logits(g, k, h, w, regime) for k in counts])
    b = Bufs(dev)
    dxl = b.operand(x)
    mk = lambda t: (out_nan(b, t + '_prob', (nobj + G, H, W)), out_nan(b, t + '_lup', (nobj + G, H, W)),
                    out_nan(b, t + '_m16', (nobj, max(ncell, 1))), sentinel_filled(b, t + '_pair', (nobj, max(ncell, 1), 8)))
    base = 1 | (4 if md else 0)
    forms = {'sh': base}
    if md:
        forms['lanes'] = base | 16
    if uniform:
        forms['rt'] = base | 8
        if md:
            forms['rt_lanes'] = base | 8 | 16
    outs = {n: mk(n) for n in list(forms) + ['one']}
    ol = O.OpList()
    for n, fl in forms.items():
        pa, la, ma, ra = outs[n]
        ints = [counts[0] + 1, h, w, 8 if md else 0, G] if uniform else [max(counts) + 1, h, w, 8 if md else 0, G, O.pack_counts(counts)]
        ol.add(O.UP4_SOFTMAX, fl, ints, [], [dxl, pa, la] + ([ma, ra] if md else []))
    pb, lb, mb, rb = outs['one']
    for c, k in enumerate(counts):
        o = st[c] + c
        ol.add(O.UP4_SOFTMAX, base, [k + 1, h, w, 8 if md else 0, 1], [], [dxl[st[c]:], pb[o:], lb[o:]] + ([mb[st[c]:], rb[st[c]:]] if md else []))
    again = launch(ol)
    if mutate:
        mutate(SimpleNamespace(x=x, outs=outs, counts=counts, st=st, h=h, w=w))
    r = {}
    refs = [up4_fused_ref(x[st[c]:st[c] + k], mask_down=md) for c, k in enumerate(counts)]
    assert all(all_finite(ref) for ref in refs)
    for n, (pa, la, ma, ra) in outs.items():
        for c, k in enumerate(counts):
            o, ref = st[c] + c, refs[c]
            r[f'{n}.clip{c}.prob'] = chk(pa[o:o + k + 1], ref['prob'], f'{n} clip {c} prob')
            r[f'{n}.clip{c}.lup'] = chk(la[o:o + k + 1], ref['lup'], f'{n} clip {c} lup')
            if md:
                r.update({f'{n}.clip{c}.{q}': v for q, v in check_mask_down(ma[st[c]:st[c] + k].view(k, h // 4, w // 4), ra[st[c]:st[c] + k].view(k, h // 4, w // 4, 8),
                                                                           ref, 8, f'{n} clip {c}').items()})
        same_bits(pa, pb, f'clips ({n}) against one-clip launches (prob)')
        same_bits(la, lb, f'clips ({n}) against one-clip launches (logits_up)')
        if md:
            same_bits(ma, mb, f'clips ({n}) against one-clip launches (m16)')
            same_bits(ra, rb, f'clips ({n}) against one-clip launches (pair)')
        else:
            assert bool(torch.isnan(ma).all()) and bool((ra == SENT_F).all())
    return finish(b, None if mutate else again, r)


# ---- MASK_MERGE / AGG_SOFTMAX -----------------------------------------------------------------------------------------------------------
MERGE_CASES = [dict(K=K, HW=HW, regime=rg, float_mode=fm) for K in (1, 4) for HW in (255, 257) for rg in ('hard', 'plain') for fm in (False, True)]


def run_merge_agg(dev, launch, *, K, HW, regime, float_mode, mutate=None):
    """MASK_MERGE (int / float mode, pads on both sides, Kold < Knew, with and without pred) into AGG_SOFTMAX; AGG_SOFTMAX also on soft / hard planes."""
    H, W = 1, HW
    h0, w0, pl, pt = 1, HW - 5, 2, 0
    Kold, Knew = K, K + 2
    g = gen(K * 3 + HW + float_mode)
    pred = torch.softmax(torch.randn((Kold + 1, H, W), generator=g) * 3, 0)
    if float_mode:
        inmask = soft_masks(g, 2, h0, w0, regime)
        src = [-1] * Kold + [0, 1]
    else:
        inmask = torch.randint(0, 4, (h0, w0), generator=g).to(I32) * 3         # ids 0, 3, 6, 9
        src = [-1] * Kold + [3, 9]
    planes_in = soft_masks(g, K, H, W, regime)
    b = Bufs(dev)
    dsrc = b.operand(torch.tensor(src, dtype=I32))
    din, dpred = b.operand(inmask), b.operand(pred)
    kw = dict(h0=h0, w0=w0, H=H, W=W, pad_left=pl, pad_top=pt, Knew=Knew, Kold=Kold, nfloat=2 if float_mode else 0, float_mode=float_mode)
    pm, pn = out_nan(b, 'planes', (Knew, H, W)), out_nan(b, 'planes_nopred', (Knew, H, W))
    prob_m, prob_s = out_nan(b, 'prob_merged', (Knew + 1, H, W)), out_nan(b, 'prob_soft', (K + 1, H, W))
    ol = O.OpList()
    ol.mask_merge(din, dpred, dsrc, pm, **kw)
    ol.mask_merge(din, None, dsrc, pn, **kw)
    ol.agg_softmax(pm, prob_m, K=Knew, HW=HW)
    ol.agg_softmax(b.operand(planes_in), prob_s, K=K, HW=HW)
    again = launch(ol)
    if mutate:
        mutate(SimpleNamespace(planes=planes_in, prob=prob_s, K=K))
    r = {}
    for name, out, p in (('merge', pm, pred), ('merge_nopred', pn, None)):
        ref = mask_merge_ref(inmask, p, src, H=H, W=W, pl=pl, pt=pt, Kold=Kold, float_mode=float_mode)
        r[name] = chk(out, ref['planes'], 'mask_merge ' + name)
    for name, planes, prob in (('agg_merged', pm, prob_m), ('agg', planes_in, prob_s)):
        ref = agg_softmax_ref(planes)
        assert all_finite(ref)
        r[name] = chk(prob, ref['prob'], 'agg_softmax ' + name)
    return finish(b, None if mutate else again, r)


RUNNERS = dict(maxpool=(run_maxpool, MAXPOOL_CASES), img_prep=(run_img_prep, IMG_PREP_CASES), upsample=(run_upsample, UPSAMPLE_CASES),
               area=(run_area, AREA_CASES), mask_down=(run_mask_down, MASK_DOWN_CASES), gap_eca=(run_gap_eca, GAP_CASES), gru=(run_gru, GRU_CASES),
               up4=(run_up4, UP4_CASES), seg_plain=(run_seg_plain, PLAIN_CASES), up4_clips=(run_up4_clips, CLIP_CASES), merge_agg=(run_merge_agg, MERGE_CASES))
ALL_CASES = [(op, kw) for op, (_, cases) in RUNNERS.items() for kw in cases]


def case_id(c):
    op, kw = c
    return op + '-' + '-'.join(f'{k}{"x".join(map(str, v)) if isinstance(v, tuple) else v}' for k, v in kw.items())


def show(op, kw, ratios):
    """The line every test prints: the worst |err| / bound per output group."""
    grp = {}
    for k, v in ratios.items():
        key = k.split('.')[-1]
        grp[key] = max(grp.get(key, 0.0), v)
    print('px_ref64 ratio', case_id((op, kw)), ' '.join(f'{k}={v:.3g}' for k, v in grp.items()))
    return max(ratios.values()) if ratios else 0.0
