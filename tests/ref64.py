"""Float64 reference of the CONV descriptor (include/cutie_hip.h CUTIE_OP_CONV) with a per-element error bound.  TEST INFRASTRUCTURE ONLY.

Independent of tests/mock_exec.py and of the kernels: the output rows are gathered pixel by pixel from the descriptor's own
addressing rules (NHWC with row strides ldx1 / ldx2, packed weights k = (kh*KW + kw)*Cin + c, residual plain / broadcast /
grouped per clip by f0 / f1, output row stride ldy) and summed in float64 from the exact bf16 operands.

The bound (``conv_ref64`` returns it next to y64) covers every fp32 kernel of the family whatever order it sums in:

  * accumulation: the Kpad bf16 x bf16 products are exact in fp32; together with the bias and the residual an output is a sum of
    at most n = Kpad + 2 terms, formed along a path of at most n - 1 fp32 roundings of relative error <= u = 2^-24 each (round to
    nearest: the MFMA accumulates in fp32, split-K slices, the WK groups of a block and the split-K reduce only reorder the sum).
    Any such order is within gamma_n * sum |terms|, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability, Lemma 3.1 / 3.4),
    sum |terms| = sum_k |x_k w_k| + |bias| + |res|.  The float64 sum's own error (n 2^-53 of the same sum) is added.
  * activation: the pre-activation error E passes through the Lipschitz factor -- ReLU 1, sigmoid 1/4, SQ1 (v*v + 1) 2|v| + E --
    plus the activation's own fp32 evaluation: sigmoid 1 / (1 + exp(-v)) with the fast exp (2^(v log2 e): the product's rounding
    is a relative error |v| u of exp, v_exp_f32 and the reciprocal 1 ulp each, the add half an ulp): <= (|v| / 4 + 4) u absolute;
    SQ1: two roundings of v*v + 1.
  * output rounding: half an ulp of the stored format, <= 2^-8 |y| (bf16) or 2^-24 |y| (fp32), of |y| + the error above.
  * flush of denormals: up to 2^-126 per rounding step, (n + 4) 2^-126 absolute (negligible, but keeps the bound sound at zero).

Rows: ``sample_rows`` picks the output rows worth checking on a large map (image borders, both sides of every BM-row tile boundary
and of every halo-patch boundary, the last ragged tile, random rows).  Works on host or device tensors alike (torch float64).
"""
import torch

U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
U64 = 2.0 ** -53
FTZ = 2.0 ** -126
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SQ1 = 0, 1, 2, 3
F_RELU_IN, F_OUT_F32, F_RES_BCAST = 1, 2, 4
ACT_SHIFT = 4


class ConvGeom:
    """The integer / float fields of a CONV descriptor that the arithmetic depends on."""
    __slots__ = ('B', 'H', 'W', 'C1', 'C2', 'ldx1', 'ldx2', 'OH', 'OW', 'Cout', 'ldy', 'KH', 'KW', 'stride', 'pad', 'ldr', 'Kpad',
                 'relu_in', 'out_f32', 'res_bcast', 'act', 'f0', 'f1')

    def __init__(self, *, B, H, W, C1, OH, OW, Cout, KH, KW, Kpad, C2=0, ldx1=None, ldx2=None, ldy=None, stride=1, pad=0, ldr=None,
                 relu_in=False, out_f32=False, res_bcast=False, act=ACT_NONE, f0=0, f1=0):
        self.B, self.H, self.W, self.C1, self.C2 = B, H, W, C1, C2
        self.ldx1, self.ldx2 = ldx1 or C1, ldx2 or C2
        self.OH, self.OW, self.Cout, self.ldy = OH, OW, Cout, ldy or Cout
        self.KH, self.KW, self.stride, self.pad, self.ldr, self.Kpad = KH, KW, stride, pad, ldr or Cout, Kpad
        self.relu_in, self.out_f32, self.res_bcast, self.act = bool(relu_in), bool(out_f32), bool(res_bcast), int(act)
        self.f0, self.f1 = int(f0), int(f1)

    @classmethod
    def from_desc(cls, i, flags, f=(0.0, 0.0)):
        """From a descriptor's i[] / flags / f[] (one record of OpList.finalize())."""
        i = [int(v) for v in i]
        flags = int(flags)
        return cls(B=i[0], H=i[1], W=i[2], C1=i[3], C2=i[4], ldx1=i[5], ldx2=i[6], OH=i[7], OW=i[8], Cout=i[9], ldy=i[10], KH=i[11], KW=i[12],
                   stride=i[13], pad=i[14], ldr=i[15], Kpad=i[16], relu_in=flags & F_RELU_IN, out_f32=flags & F_OUT_F32,
                   res_bcast=flags & F_RES_BCAST, act=(flags >> ACT_SHIFT) & 7, f0=int(f[0]) if flags & F_RES_BCAST else 0, f1=int(f[1]))

    @property
    def Cin(self):
        return self.C1 + self.C2

    @property
    def M(self):
        return self.B * self.OH * self.OW

    @property
    def OHW(self):
        return self.OH * self.OW

    def res_rows(self, m):
        """Residual row that output row m adds (conv_common.h conv_res_row)."""
        if not self.res_bcast:
            return m
        r = m % self.OHW
        if self.f0 > 0:
            r = r + (m // (self.f0 * self.OHW)) * self.f1
        return r

    def res_extent(self):
        """Rows a residual buffer must hold."""
        if not self.res_bcast:
            return self.M
        if self.f0 > 0:
            return (self.B // self.f0 - 1) * self.f1 + self.OHW
        return self.OHW


def sample_rows(g, *, bm=None, halo=None, n_random=2048, seed=0, device='cpu'):
    """Output rows to check: every image-border pixel, both sides of every BM-row tile boundary (bm), of every halo patch
    boundary (halo = (TH, TW) of tiles 120..), the whole last ragged tile, and n_random random rows.  Sorted, unique, int64."""
    M, OH, OW = g.M, g.OH, g.OW
    m = torch.arange(M, dtype=torch.int64)
    oh, ow = (m % g.OHW) // OW, m % OW
    keep = (oh == 0) | (oh == OH - 1) | (ow == 0) | (ow == OW - 1)
    if bm:
        r = m % bm
        keep |= (r == 0) | (r == bm - 1)
        keep |= m >= (M // bm) * bm                                       # the last ragged tile (M % bm rows), whole
        keep |= m >= M - bm                                               # ... and the last full one
    if halo:
        th, tw = halo
        keep |= (oh % th == 0) | (oh % th == th - 1) | (ow % tw == 0) | (ow % tw == tw - 1)
        keep |= (oh >= (OH // th) * th) | (ow >= (OW // tw) * tw)        # ragged patches
    gen = torch.Generator().manual_seed(seed)
    if n_random:
        keep[torch.randint(0, M, (min(n_random, M),), generator=gen)] = True
    return m[keep].to(device)


def _gather(g, x1, x2, rows, dev):
    """im2col of the given output rows in float64: [R, KH*KW*Cin] in packed-k order (zeros outside the image)."""
    b = rows // g.OHW
    oh = (rows % g.OHW) // g.OW
    ow = rows % g.OW
    cols = []
    for kh in range(g.KH):
        for kw in range(g.KW):
            ih = oh * g.stride - g.pad + kh
            iw = ow * g.stride - g.pad + kw
            inside = (ih >= 0) & (ih < g.H) & (iw >= 0) & (iw < g.W)
            pix = (b * g.H + ih.clamp(0, g.H - 1)) * g.W + iw.clamp(0, g.W - 1)
            parts = [x1[pix][:, :g.C1]]
            if g.C2:
                parts.append(x2[pix][:, :g.C2])
            v = torch.cat(parts, 1).to(torch.float64)
            v = torch.where(inside.view(-1, 1), v, torch.zeros((), dtype=torch.float64, device=dev))
            cols.append(v)
    a = torch.cat(cols, 1)
    if g.relu_in:
        a = a.clamp(min=0)
    return a


def _act64(z, act):
    if act == ACT_RELU:
        return z.clamp(min=0)
    if act == ACT_SIGMOID:
        return torch.sigmoid(z)
    if act == ACT_SQ1:
        return z * z + 1
    return z


def conv_ref64(g, x1, w, *, x2=None, bias=None, res=None, rows=None, chunk_elems=1 << 25):
    """y64 [R, Cout] and its per-element error bound [R, Cout] (float64) for the output rows `rows` (flat indices into [B, OH, OW];
    None = all).  x1 / x2: pixel-major tensors of B*H*W rows of ldx1 / ldx2 bf16 values ([B, H, W, ldx] or any view of that
    layout); w: packed bf16 [CoutPad, Kpad]; bias f32 [Cout] or None; res: rows of ldr bf16 values addressed by ConvGeom.res_rows."""
    dev = x1.device
    x1 = x1.reshape(-1, g.ldx1)
    x2 = x2.reshape(-1, g.ldx2) if g.C2 else None
    if rows is None:
        rows = torch.arange(g.M, dtype=torch.int64, device=dev)
    rows = rows.to(dev)
    K = g.KH * g.KW * g.Cin
    wm = w.reshape(-1, g.Kpad)[:g.Cout, :K].to(torch.float64)
    assert torch.isfinite(wm).all()
    wa = wm.abs().t().contiguous()
    wm = wm.t().contiguous()
    n = g.Kpad + 2
    gamma = n * U32 / (1 - n * U32) + n * U64
    b64 = bias.to(dev, torch.float64).view(1, -1)[:, :g.Cout] if bias is not None else None
    resv = res.reshape(-1, g.ldr)[:, :g.Cout] if res is not None else None
    ys, bs = [], []
    step = max(1, chunk_elems // max(K, 1))
    for s in range(0, len(rows), step):
        r = rows[s:s + step]
        a = _gather(g, x1, x2, r, dev)
        z = a @ wm
        mag = a.abs() @ wa
        if b64 is not None:
            z = z + b64
            mag = mag + b64.abs()
        if resv is not None:
            rv = resv[g.res_rows(r)].to(torch.float64)
            z = z + rv
            mag = mag + rv.abs()
        e = gamma * mag + (n + 4) * FTZ
        y = _act64(z, g.act)
        if g.act == ACT_SIGMOID:
            e = e / 4 + (z.abs() / 4 + 4) * U32
        elif g.act == ACT_SQ1:
            e = e * (2 * z.abs() + e) + 2 * U32 * (z * z + 1)
        e = e + (U32 if g.out_f32 else U_BF16) * (y.abs() + e)
        ys.append(y)
        bs.append(e)
    return torch.cat(ys), torch.cat(bs)


def stored_rows(g, y, rows):
    """The kernel's stored values of `rows` as float64 [R, Cout] from an output buffer of M rows of ldy values."""
    return y.reshape(-1)[:g.M * g.ldy].view(g.M, g.ldy)[rows.to(y.device), :g.Cout].to(torch.float64)


def check_bound(got, y64, bound, what=''):
    """Every element within its bound (NaN anywhere fails).  Returns the worst |got - y64| / bound."""
    d = (got.to(torch.float64) - y64).abs()
    ratio = d / bound
    bad = ~(d <= bound)
    if bool(bad.any()):
        k = int(bad.view(-1).nonzero()[0])
        r, c = divmod(k, y64.shape[1])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements outside the float64 bound; first at sampled row {r} channel {c}: '
                             f'got {float(got[r, c])} ref {float(y64[r, c])} bound {float(bound[r, c]):.3g}')
    return float(ratio.max()) if ratio.numel() else 0.0


GAP_LIMIT = 2.0 ** 20


def gap_fixed(v):
    """The GAP side job's fixed point of stored values (conv_common.h conv_gapfx): round(v * 2^20) to nearest even,
    exact for |v| <= 2^20; larger magnitudes (infinities included) saturate at +-2^40, NaN counts as 0.  int64."""
    v = v.to(torch.float64)
    q = torch.round(v.clamp(-GAP_LIMIT, GAP_LIMIT) * 1048576.0)
    q = torch.where(torch.isnan(v), torch.zeros_like(q), q)
    return q.to(torch.int64)


def operand(gen, rows, C, *, regime='randn', ld=None, scale=0.5, fill=0.0):
    """rows x ld bf16 activations (channels [C, ld) = fill):
    'randn' -- randn * scale;  'sparse' -- post-ReLU (about a third of the values non-zero) with per-channel scales log-uniform in
    [2^-6, 2^6], the production-like regime where a fault in a small channel hides behind the large ones."""
    ld = ld or C
    dev = gen.device
    v = torch.randn(rows, C, generator=gen, device=dev)
    if regime == 'sparse':
        v = (v - 0.45).clamp(min=0) * torch.exp2(torch.rand(C, generator=gen, device=dev) * 12 - 6)
    elif regime == 'randn':
        v = v * scale
    else:
        raise ValueError(regime)
    out = torch.full((rows, ld), fill, dtype=torch.bfloat16, device=dev)
    out[:, :C] = v.to(torch.bfloat16)
    return out
