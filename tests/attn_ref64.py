"""Float64 references of the object transformer's query side (csrc/attention.hip, csrc/qchain.hip: AUX_MASK, ATTN_Q2P, ATTN_SELF, ATTN_P2Q,
QFFN, QUERY_INIT with its linears) with a per-element error bound.  TEST INFRASTRUCTURE ONLY.

Independent of tests/mock_exec.py and of the kernels: written from the descriptors (include/cutie_hip.h, cutie_amd/ops.py) and the kernels'
comments, in plain torch float64 from the exact bf16 / fp32 / int64 operand values of ONE launch, with that launch's strides and layouts
(pixel rows of ldkv values with k at head * hstride and v at voff + head * hstride; fixed-point accumulators int64 x 2^32).  Every function
returns (y64, bound) pairs of one shape; host or device tensors alike.

The bound, first order in the unit roundoffs (second-order terms are below 2^-40 of the first-order ones and are covered by the explicit
(1 + eta) factors where a term could be large), from these ingredients:

  * bf16 x bf16 products are exact in fp32 (8 + 8 significand bits), so an MFMA step only rounds when it accumulates.
  * split operands: x = hi + lo + r with hi = bf16(x), lo = bf16(x - hi), |r| <= u_bf16^2 |x| (SPLIT), u_bf16 = 2^-8 as in ref64.py
    (split_bf2 in attention_common.h).  A product of two split operands without the lo . lo term (mfma3 in qchain.hip) loses another
    u_bf16^2 |a||b|: 3 SPLIT in all.  |hi| + |lo| <= (1 + 2 u_bf16)|x| enters the sum of magnitudes.
  * fp32 accumulation of n terms in ANY order is within gamma_n sum|terms|, gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Lemma 3.1; the
    same lemma ref64.py uses).  The LDS merges of k-steps and waves only reorder the sum; n counts every add and every rescale on a path.
  * __expf(x) = v_exp_f32(x log2 e): the subtraction in front, the product and the rounded constant perturb exp by a relative 3|x|u, the
    instruction by one ulp (2u) -- the assumptions ref64.py makes for the fast sigmoid.  __frcp_rn / rsqrtf / 1.f / x: one ulp (2u).
  * softmax: the kernel's weights w^_j (any common shift cancels in the quotient) satisfy |w^_j - w_j| <= eps_j = w_j eta_j + 2 FTZ with
    eta_j = expm1(E_s,j) + (3 (M - s_j + 2 max E_s) + 3 n_exp + 2) u: the score error E_s, the distance to the maximum travelled in
    n_exp exponentials (the online rescales alpha of ATTN_Q2P and the merge factor multiply up to exactly M - s_j).  With N = sum w v,
    D = sum w:  |N^/D^ - N/D| <= (|N^ - N| + |o||D^ - D|) / (D - |D^ - D|).  For uniform E_s and eta this is the textbook
    2 eta / (1 - eta) sum_j p_j |v_j|; the per-element form stays sharp where a few pixels carry all the weight.
  * two-pass LayerNorm in fp32: mean (gamma_256), centred values, variance, rsqrtf, scale and shift, each step's rounding propagated; an
    input perturbation E goes through the Jacobian |g_i| rstd (E_i + mean E + |xhat_i| mean(|xhat| E)), inflated by (1 + 4 rstd max E).
  * fixed point: qacc_add rounds v 2^32 (exact in fp32) to the nearest integer: 2^-33 per addend, times the number of addends of a launch
    (8 heads; FF / hid_slice slices); integer sums are exact.  Reading an accumulator back (x_eff = x + abias + acc / 2^32) costs the
    int64 -> fp32 rounding and two adds.
  * stored outputs: half an ulp of the format (2^-8 |y| bf16, 2^-24 |y| fp32 -- the latter is part of the last operation's rounding).
  * flush of denormals: a few 2^-126 per step (FTZ), which keeps the bound sound at zero.
Stage errors propagate through the next stage's Lipschitz factor evaluated on the float64 data (|W| for a projection, the Jacobian of
LayerNorm, expm1 for the softmax), as conv_ref64 does for activations.

Mask decisions (mask_ref64): fg[k, p] = L_k >= max(L_bg, max_j L_j), L = logit(clamp(p, 1e-7, 1 - 1e-7)), p_j = sigmoid(logit_j), p_bg =
prod (1 - p_j).  logit is increasing, so the clamped probabilities are compared.  The returned margin is the smallest relative distance
between two compared values of a pixel (inf where both sit on the same clamp: an exact tie, foreground in every form); the tests only use
logits whose margin is at least MASK_MARGIN everywhere, so that the fast sigmoid of the kernels decides like this form.

`mut`: names of faults applied to the float64 computation itself (tests/test_attn_ref64_cpu.py shows that the bound catches them).
"""
import math

import torch

from ref64 import U32, U_BF16, U64, FTZ

SPLIT = U_BF16 * U_BF16
QSCALE = 4294967296.0
RSQ32 = 1.0 / math.sqrt(32.0)
FIX = 2.0 ** -33                  # one qacc_add
MASK_MARGIN = 1e-4
LN_EPS = float(torch.tensor(1e-5, dtype=torch.float32).double())
P_LO = float(torch.tensor(1e-7, dtype=torch.float32).double())
P_HI = float((torch.tensor(1.0, dtype=torch.float32) - torch.tensor(1e-7, dtype=torch.float32)).double())
HEADS, HD, C, Q = 8, 32, 256, 16
F64 = torch.float64


def gam(n):
    return n * U32 / (1 - n * U32) + n * U64


def hi_bf16(x):
    """What is left of a split operand when its lo half is dropped."""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def rows_of(buf, n, ld, ncols, off=0):
    """n rows of ncols values at row stride ld from element `off` of a buffer (any dtype; the gaps are never read)."""
    flat = buf.reshape(-1)
    return torch.as_strided(flat, (n, ncols), (ld, 1), flat.storage_offset() + off)


def heads_of(buf, K, N, ld, off, hstride):
    """[K, 8, N, 32] float64: the 32 values of head h of row (k, n) at column off + h * hstride."""
    rows = rows_of(buf, K * N, ld, off + 7 * hstride + HD)
    col = (off + hstride * torch.arange(HEADS, device=buf.device).view(-1, 1) + torch.arange(HD, device=buf.device).view(1, -1)).reshape(-1)
    return rows[:, col].to(F64).view(K, N, HEADS, HD).permute(0, 2, 1, 3)


# ---- mask -----------------------------------------------------------------------------------------------------------------------------
def mask_ref64(lg, Kg=None):
    """lg f32 [K, HW]; Kg: objects per clip.  -> fg bool [K, HW], margin float64 [K, HW]."""
    K, HW = lg.shape
    Kg = Kg or K
    x = lg.to(F64).view(K // Kg, Kg, HW)
    pr = torch.sigmoid(x)
    om = torch.where(x > 0, torch.exp(-x) / (1 + torch.exp(-x)), 1 / (1 + torch.exp(x)))          # 1 - p without cancellation
    bg = om.prod(1, keepdim=True).clamp(P_LO, P_HI)
    pc = pr.clamp(P_LO, P_HI)

    def rel(a, b):
        d = (a - b).abs() / torch.maximum(a, b)
        return torch.where(a == b, torch.full_like(d, float('inf')), d)
    fg = pc >= bg
    margin = rel(pc, bg.expand_as(pc))
    for j in range(Kg):
        other = pc[:, j:j + 1]
        notself = torch.ones(Kg, dtype=torch.bool, device=lg.device)
        notself[j] = False
        fg = fg & ((pc >= other) | ~notself.view(1, -1, 1))
        margin = torch.where(notself.view(1, -1, 1), torch.minimum(margin, rel(pc, other.expand_as(pc))), margin)
    return fg.reshape(K, HW), margin.reshape(K, HW)


def mask_logits(gen, K, HW, *, Kg=None, sat=None, n_fg=None, scale=2.0):
    """Logits f32 [K, HW] without a borderline pixel: randn * scale clamped to |logit| <= 12; sat = {object: +-20 | +-30} saturates whole
    planes; n_fg = {object: n}: object's foreground is exactly n pixels, pixel 0 and pixel HW - 1 among them when n allows (planes of the
    same clip as such an object are pushed down there).  Offending pixels are redrawn on a grid of distinct values; the result is asserted
    to have a margin >= MASK_MARGIN everywhere (zero excluded pixels)."""
    Kg = Kg or K
    lg = (torch.randn((K, HW), generator=gen) * scale).clamp(-12, 12)
    sat = dict(sat or {})
    unsat = torch.ones(K, dtype=torch.bool)
    for k, v in sat.items():
        lg[k] = float(v)
        unsat[k] = False
    for k, n in (n_fg or {}).items():
        c0 = (k // Kg) * Kg
        on = torch.zeros(HW, dtype=torch.bool)
        if n >= HW:
            on[:] = True
        elif n > 0:
            pick = [HW - 1, 0][:n]
            rest = [p for p in torch.randperm(HW, generator=gen).tolist() if p not in (0, HW - 1)]
            on[torch.tensor(pick + rest[:n - len(pick)], dtype=torch.int64)] = True
        for j in range(c0, c0 + Kg):
            if j == k:
                lg[j] = torch.where(on, lg[j].abs() + 1.0, -lg[j].abs() - 6.0).clamp(-12, 12)
            elif unsat[j]:
                lg[j] = torch.where(on, -lg[j].abs() - 3.5, lg[j]).clamp(-12, 12)
    for it in range(8):
        _, margin = mask_ref64(lg, Kg)
        bad = (margin < MASK_MARGIN).view(K // Kg, Kg, HW).any(1)                                  # [clips, HW]
        if not bool(bad.any()):
            break
        for k in range(K):
            if unsat[k] and not (n_fg and k in n_fg):
                b = bad[k // Kg]
                p = b.nonzero().view(-1)
                # distinct values per plane; under a plane whose foreground is prescribed they stay below every value that plane takes there
                base, step = (-11.5, 0.8) if (n_fg and any(j // Kg == k // Kg for j in n_fg)) else (-6.0, 0.9)
                lg[k, p] = (base + step * (((k % Kg) * 7 + p + 3 * it) % 11) + 0.037 * it).to(lg.dtype)
    fg, margin = mask_ref64(lg, Kg)
    assert float(margin.min()) >= MASK_MARGIN, 'mask_logits: a borderline pixel is left'
    for k, n in (n_fg or {}).items():
        assert int(fg[k].sum()) == min(n, HW), ('mask_logits: foreground count', k, n, int(fg[k].sum()))
    return lg


# ---- rows, LayerNorm, projections ---------------------------------------------------------------------------------------------------
def eff_rows(x, acc=None, abias=None, mut=()):
    """x_eff = x + abias + acc / 2^32 of [M, 256] rows (fp32 x, int64 acc, fp32 abias) -> (v, E)."""
    v = x.to(F64)
    E = torch.zeros_like(v)
    if acc is not None:
        a = acc.to(F64) / QSCALE
        ab = abias.to(F64).view(1, -1) if (abias is not None and 'no_abias' not in mut) else torch.zeros((), dtype=F64, device=x.device)
        E = U32 * a.abs() + gam(2) * (v.abs() + ab.abs() + a.abs()) + 3 * FTZ      # int64 -> fp32, then two adds in either order
        v = v + (ab + a)
    return v, E


def layernorm(v, E, g, b):
    g, b = g.to(F64).view(1, -1), b.to(F64).view(1, -1)
    n = v.shape[-1]
    mean = v.mean(-1, keepdim=True)
    d = v - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(var + LN_EPS)
    xh = d * rstd
    y = xh * g + b
    dm = gam(n) * v.abs().mean(-1, keepdim=True)
    dd = dm + U32 * d.abs()
    dvar = 2 * (d.abs() * dd).mean(-1, keepdim=True) + gam(n + 2) * var
    rho = (dvar + U32 * (var + LN_EPS)) / (2 * (var + LN_EPS)) + 2 * U32
    Ey = g.abs() * (dd * rstd + xh.abs() * (rho + 2 * U32)) + U32 * y.abs() + 4 * FTZ
    lip = g.abs() * rstd * (E + E.mean(-1, keepdim=True) + xh.abs() * (xh.abs() * E).mean(-1, keepdim=True))
    lip = lip * (1 + 4 * rstd * E.max(-1, keepdim=True).values)
    return y, Ey + lip


def add_rows(v, E, add):
    y = v + add.to(F64)
    return y, E + U32 * y.abs()


def proj(xs, Ex, W, bias=None, *, scale=None, extra=None, drop_lo=False, nsplit=1, n=None):
    """y = xs . W^T (+ bias) (+ extra) (* scale): xs float64 [M, Kd] with error Ex, split hi + lo on bf16 MFMA; W bf16 [N, Kd] rows."""
    Wd = W.to(F64)
    Kd = Wd.shape[1]
    xv = hi_bf16(xs) if drop_lo else xs
    y = xv @ Wd.t()
    mag = (xs.abs() @ Wd.abs().t()) * (1 + 2 * U_BF16)
    n = n or 2 * Kd + 4                                              # hi and lo products of every k, bias / residual, the merges
    for t in (bias, extra):
        if t is not None:
            t = t.to(F64)
            t = t.view(1, -1) if t.dim() == 1 else t
            y = y + t
            mag = mag + t.abs()
    E = Ex @ Wd.abs().t() + (nsplit * SPLIT + gam(n)) * mag + (n + 4) * FTZ
    if scale is not None:
        y = y * scale
        E = E * scale + 3 * U32 * y.abs()
    return y, E


def softmax_av(s, Es, v, Ev, *, allowed=None, rel_pv, n_acc, n_exp, drop_pl=False, drop_vl=False):
    """o = softmax(s) v over the last axis of s [..., R, N] (scores with error Es), v [..., N, D] (error Ev or None) -> (o, E)."""
    if allowed is not None:
        s = torch.where(allowed, s, torch.full_like(s, float('-inf')))
        Es = torch.where(allowed, Es, torch.zeros_like(Es))
    M = s.max(-1, keepdim=True).values
    dist = M - s
    w = torch.exp(-dist)
    live = torch.isfinite(dist)
    Esm = Es.max(-1, keepdim=True).values
    eta = torch.expm1(Es) + (3 * (dist + 2 * Esm) + 3 * n_exp + 2) * U32
    eps = torch.where(live, w * eta + 2 * FTZ, torch.zeros_like(w))
    D = w.sum(-1, keepdim=True)
    av = v.abs()
    o = ((hi_bf16(w) if drop_pl else w) @ (hi_bf16(v) if drop_vl else v)) / D
    g = gam(n_acc)
    eN = (eps + (w + eps) * (rel_pv + g)) @ av
    if Ev is not None:
        eN = eN + (w + eps) @ Ev
    eD = eps.sum(-1, keepdim=True) + g * D
    E = (eN + o.abs() * eD) / (D - eD) + 4 * U32 * o.abs() + 4 * FTZ
    return o, E


def _heads(x):                                      # [K*16, 256] -> [K, 8, 16, 32]
    return x.view(-1, Q, HEADS, HD).permute(0, 2, 1, 3)


def _unheads(x):                                    # [K, 8, R, 32] -> [K*R, 256]
    return x.permute(0, 2, 1, 3).reshape(-1, C)


def scores(q, Eq, k, Ek, *, nsplit, n):
    """s[r, j] = q_r . k_j over 32 dims on MFMA / in fp32: (s, Es)."""
    s = q @ k.transpose(-1, -2)
    mag = (q.abs() @ k.abs().transpose(-1, -2)) * (1 + 2 * U_BF16)
    Es = (nsplit * SPLIT + gam(n)) * mag + (n + 4) * FTZ
    if Eq is not None:
        Es = Es + Eq @ k.abs().transpose(-1, -2)
    if Ek is not None:
        Es = Es + (q.abs() + (Eq if Eq is not None else 0)) @ Ek.transpose(-1, -2)
    return s, Es


def out_proj_acc(o, Eo, Wo, acc0, *, naddends, mut=(), ksplit=HD):
    """acc / 2^32 after the launch: acc0 / 2^32 + o . Wo^T, one fixed-point addend per (element, k-slice of ksplit columns)."""
    od = o
    if 'drop_ol' in mut:
        od = hi_bf16(o)
    if 'head_missing' in mut:
        od = od.clone()
        od[:, 3 * ksplit:4 * ksplit] = 0
    a, E = proj(od, Eo, Wo, n=2 * ksplit + 2)                            # each addend is a sum over its own ksplit columns only
    E = E + naddends * (FIX + 8 * FTZ)
    base = acc0.to(F64) / QSCALE if acc0 is not None else 0.0
    return base + a, E


# ---- ATTN_Q2P ---------------------------------------------------------------------------------------------------------------------------
def q2p_ref64(kv, *, K, HW, ldkv, voff, hstride=HD, q=None, q_pre=None, proj_in=None, fg=None, nfg=None, lg=None, Kg=None, out=None, mut=()):
    """Masked cross attention of the 16 queries of K objects over HW pixels.
    kv: bf16 pixel rows (ldkv values; k of head h at h * hstride, v at voff + h * hstride).
    q f32 [K*16, 256] (scaled in the launch) | q_pre f32 (projected and scaled beforehand) |
    proj_in = dict(x, W, bias, emb, ln_g, ln_b, acc=None, abias=None): q = ((LN(x_eff) + emb) W^T + b) / sqrt(32).
    fg uint8 [K, HW] + nfg int32 [K] | lg f32 [K, HW] (+ Kg objects per clip).  out = dict(Wo, acc0): chain form.
    -> dict: 'y' (attention output [K*16, 256]), 'acc' (chain form, in units of 1), 'ln_out', 'fg' (bool), 'n_fg'; floats as (y64, bound)."""
    mut = frozenset(mut)
    dev = kv.device
    res = {}
    if 'layout_swap' in mut:
        voff, hstride = (HD, 2 * HD) if hstride == HD else (C, HD)
    if q_pre is not None:
        qf, Eq = q_pre.to(F64).view(-1, C), None
        if 'scale_twice' in mut:
            qf = qf * RSQ32
    elif proj_in is not None:
        p = proj_in
        v, E = eff_rows(p['x'], p.get('acc'), p.get('abias'), mut)
        xn, Exn = layernorm(v, E, p['ln_g'], p['ln_b'])
        res['ln_out'] = (xn, Exn)
        xa, Exa = add_rows(xn, Exn, p['emb'])
        qf, Eq = proj(xa, Exa, p['W'], p['bias'], scale=RSQ32, drop_lo='drop_xl' in mut)
    else:
        qf = q.to(F64).view(-1, C) * RSQ32
        Eq = 3 * U32 * qf.abs()
    if 'drop_ql' in mut:
        qf = hi_bf16(qf)
    if lg is not None:
        fgb, margin = mask_ref64(lg, Kg)
        n_fg = fgb.sum(1)
        res['margin'] = margin
    else:
        fgb, n_fg = fg.view(K, HW) != 0, nfg.to(torch.int64)
    res['fg'], res['n_fg'] = fgb, n_fg
    if 'mask_shift' in mut:
        fgb = torch.roll(fgb, 1, 1)
    isfg = (torch.arange(Q, device=dev) < Q // 2).view(1, Q, 1)
    if 'swap_halves' in mut:
        isfg = ~isfg
    masked = torch.where(isfg, (n_fg != 0).view(K, 1, 1), (n_fg != HW).view(K, 1, 1))
    if 'no_unblock' in mut:
        masked = torch.ones_like(masked)
    allowed = (~masked | (fgb.view(K, 1, HW) == isfg)).view(K, 1, Q, HW)
    kh = heads_of(kv, K, HW, ldkv, 0, hstride)
    vh = heads_of(kv, K, HW, ldkv, voff, hstride)
    if 'skip_chunk' in mut:
        c0 = 32 * (((HW + 31) // 32) // 2)
        allowed = allowed.clone().expand(K, 1, Q, HW).clone()
        allowed[..., c0:c0 + 32] = False
    if 'pad_dup' in mut:
        kh, vh = torch.cat([kh, kh[:, :, -1:]], 2), torch.cat([vh, vh[:, :, -1:]], 2)
        allowed = torch.cat([allowed.expand(K, 1, Q, HW), allowed.expand(K, 1, Q, HW)[..., -1:]], -1)
    qh = _heads(qf)
    s, Es = scores(qh, None if Eq is None else _heads(Eq), kh, None, nsplit=1, n=2 * HD + 1)
    cpw = -(-((HW + 31) // 32) // 8)                                 # chunks per wave at 8 waves (the 16-wave kernel has fewer)
    o, Eo = softmax_av(s, Es, vh, None, allowed=allowed.expand(K, HEADS, Q, allowed.shape[-1]), rel_pv=SPLIT, n_acc=65 * cpw + 24, n_exp=cpw + 2,
                       drop_pl='drop_pl' in mut)
    y, Ey = _unheads(o), _unheads(Eo)
    res['y'] = (y, Ey)
    if out is not None:
        res['acc'] = out_proj_acc(y, Ey, out['Wo'], out.get('acc0'), naddends=HEADS, mut=mut)
    return res


# ---- ATTN_SELF --------------------------------------------------------------------------------------------------------------------------
def self_ref64(*, K, qk=None, v=None, ldqk=2 * C, ldv=C, proj_in=None, out=None, mut=()):
    """16 x 16 self attention per object and head.  Plain: qk f32 rows [q | k] (row stride ldqk), v f32 rows (ldv).
    proj_in = dict(x, W [768, 256], bias, emb, ln_g, ln_b, acc=None, abias=None): q, k from LN(x_eff) + emb, v from LN(x_eff).
    out = dict(Wo, acc0): chain form (MFMA attention with both operands split, output projection into the accumulator)."""
    mut = frozenset(mut)
    res = {}
    chain = out is not None
    if proj_in is not None:
        p = proj_in
        xv, E = eff_rows(p['x'], p.get('acc'), p.get('abias'), mut)
        xn, Exn = layernorm(xv, E, p['ln_g'], p['ln_b'])
        res['ln_out'] = (xn, Exn)
        xa, Exa = add_rows(xn, Exn, p['emb'])
        W, b = p['W'], p['bias']
        dl = 'drop_xl' in mut
        qf, Eq = proj(xa, Exa, W[:C], b[:C], scale=RSQ32, drop_lo=dl)
        kf, Ek = proj(xa, Exa, W[C:2 * C], b[C:2 * C], drop_lo=dl)
        if 'emb_on_v' in mut:
            vf, Ev = proj(xa, Exa, W[2 * C:3 * C], b[2 * C:3 * C], drop_lo=dl)
        else:
            vf, Ev = proj(xn, Exn, W[2 * C:3 * C], b[2 * C:3 * C], drop_lo=dl)
    else:
        qf = rows_of(qk, K * Q, ldqk, C).to(F64) * RSQ32
        Eq = 3 * U32 * qf.abs()
        kf, Ek = rows_of(qk, K * Q, ldqk, C, C).to(F64), None
        vf, Ev = rows_of(v, K * Q, ldv, C).to(F64), None
    if 'drop_ql' in mut:
        qf = hi_bf16(qf)
    if 'drop_kl' in mut:
        kf = hi_bf16(kf)
    s, Es = scores(_heads(qf), _heads(Eq), _heads(kf), None if Ek is None else _heads(Ek), nsplit=3 if chain else 0, n=3 * HD + 4)
    o, Eo = softmax_av(s, Es, _heads(vf), None if Ev is None else _heads(Ev), rel_pv=3 * SPLIT if chain else 0.0, n_acc=3 * Q + 24, n_exp=1,
                       drop_pl='drop_pl' in mut, drop_vl='drop_vl' in mut)
    y, Ey = _unheads(o), _unheads(Eo)
    res['y'] = (y, Ey)
    if chain:
        res['acc'] = out_proj_acc(y, Ey, out['Wo'], out.get('acc0'), naddends=HEADS, mut=mut)
    return res


# ---- ATTN_P2Q ---------------------------------------------------------------------------------------------------------------------------
def p2q_ref64(qpix, *, K, HW, ldq, qoff=0, kq=None, vq=None, ldkv=C, proj_in=None, next_q=None, chain=False, mut=()):
    """Cross attention of HW pixels over the 16 queries of their object, bf16 output [K*HW, 256].
    qpix: bf16 pixel rows (row stride ldq, the 256 q values at column qoff).  Plain: kq, vq f32 rows (ldkv).
    proj_in = dict(x, W [512, 256], bias, emb, acc=None, abias=None): k from x_eff + emb, v from x_eff (chain: acc given, MFMA attention).
    next_q = dict(ln_g, ln_b, W, bias): -> 'xn_out' = LN(x_eff), 'q_out' = ((xn_out + emb) W^T + b) / sqrt(32)."""
    mut = frozenset(mut)
    res = {}
    qp = heads_of(qpix, K, HW, ldq, qoff, HD)                         # [K, 8, HW, 32], exact bf16
    if proj_in is not None:
        p = proj_in
        xv, E = eff_rows(p['x'], p.get('acc'), p.get('abias'), mut)
        xa, Exa = add_rows(xv, E, p['emb'])
        W, b = p['W'], p['bias']
        dl = 'drop_xl' in mut
        kf, Ek = proj(xa, Exa, W[:C], b[:C], scale=RSQ32 if chain else None, drop_lo=dl)
        vf, Ev = proj(xa, Exa, W[C:], b[C:], drop_lo=dl) if 'emb_on_v' in mut else proj(xv, E, W[C:], b[C:], drop_lo=dl)
        if next_q is not None:
            nq = next_q
            xn, Exn = layernorm(xv, E, nq['ln_g'], nq['ln_b'])
            res['xn_out'] = (xn, Exn)
            xq, Exq = add_rows(xn, Exn, p['emb'])
            res['q_out'] = proj(xq, Exq, nq['W'], nq['bias'], scale=RSQ32, drop_lo=dl)
    else:
        kf, Ek = rows_of(kq, K * Q, ldkv, C).to(F64), None
        vf, Ev = rows_of(vq, K * Q, ldkv, C).to(F64), None
    if chain:
        if 'drop_kl' in mut:
            kf = hi_bf16(kf)
        s, Es = scores(qp, None, _heads(kf), _heads(Ek), nsplit=1, n=2 * HD + 1)
    else:
        qs = qp * RSQ32                                               # the pixel's q is scaled in fp32, the products are fp32
        s, Es = scores(qs, 3 * U32 * qs.abs(), _heads(kf), None if Ek is None else _heads(Ek), nsplit=0, n=HD + 2)
    o, Eo = softmax_av(s, Es, _heads(vf), None if Ev is None else _heads(Ev), rel_pv=3 * SPLIT if chain else 0.0, n_acc=3 * Q + 24, n_exp=1,
                       drop_pl='drop_pl' in mut, drop_vl='drop_vl' in mut)
    y, Ey = _unheads(o), _unheads(Eo)                                 # [K*HW, 256]
    res['y'] = (y, Ey + U_BF16 * (y.abs() + Ey))
    return res


# ---- QFFN -------------------------------------------------------------------------------------------------------------------------------
def qffn_ref64(x, acc_in, abias, ln_g, ln_b, W1, b1, W2, acc0, *, hid_slice, mut=()):
    """acc_out / 2^32 = acc0 / 2^32 + relu(LN(x_eff) W1^T + b1) W2^T, one addend per hidden slice; x_out = x_eff."""
    mut = frozenset(mut)
    v, E = eff_rows(x, acc_in, abias, mut)
    xn, Exn = layernorm(v, E, ln_g, ln_b)
    h, Eh = proj(xn, Exn, W1, b1, drop_lo='drop_xl' in mut)
    h = h.clamp(min=0)
    FF = W1.shape[0]
    if 'slice_missing' in mut:
        h = h.clone()
        h[:, hid_slice:2 * hid_slice] = 0
    a, Ea = proj(h, Eh, W2[:, :FF], n=2 * hid_slice + 2)
    Ea = Ea + (FF // hid_slice) * (FIX + 8 * FTZ)
    return {'x_out': (v, E), 'acc': (acc0.to(F64) / QSCALE + a, Ea)}


# ---- QUERY_INIT with its two linears ------------------------------------------------------------------------------------------------------
def query_init2_ref64(om, Wi, bi, ri, We, be, re, mut=()):
    """om f32 [M, 257] (sums | area): x = sums / (area + 1e-4); query = x Wi^T + bi + ri, query_emb = x We^T + be + re."""
    o = om.to(F64)
    eps = float(torch.tensor(1e-4, dtype=torch.float32).double())
    den = o[:, C:C + 1] + (0.0 if 'no_area_eps' in mut else eps)
    x = o[:, :C] / den
    Ex = 5 * U32 * x.abs() + 2 * FTZ
    dl = 'drop_xl' in mut
    return {'query': proj(x, Ex, Wi, bi, extra=ri, drop_lo=dl), 'query_emb': proj(x, Ex, We, be, extra=re, drop_lo=dl)}
