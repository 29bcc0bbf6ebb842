"""Launch builders for the object-transformer kernels, shared by tests/test_attn_ref64_cpu.py (the interpreter on the host) and
tests/test_gpu_attn_ref64.py (the HIP kernels).  TEST INFRASTRUCTURE ONLY.

A builder lays every operand between NaN rows (integers: between sentinel values) and every output between sentinel rows, records ONE
launch (plus AUX_MASK where asked) in an ops.OpList and returns a Case: `ref()` computes the float64 reference of attn_ref64.py from the
very buffers the launch reads, `got()` returns what the launch left in the same units, `guards_intact()` checks the sentinels, `reset()`
restores the outputs (accumulators are added to) so that a launch can be run twice.

Regimes of the operands: 'randn'; 'few' (a handful of visible pixels: masks by n_fg); 'large' (q rows x 8, every fifth projection row
x 16: score ranges of several tens); 'sparse' (rows with per-channel scales log-uniform in [2^-6, 2^6], as ref64.operand)."""
import torch

import attn_ref64 as A
from cutie_amd import ops as O
from cutie_amd.model.weights import PackedLinear

BF16, F32, I64 = torch.bfloat16, torch.float32, torch.int64
C, Q, HEADS, FF = 256, 16, 8, 2048
PAD = 512
SENT_F, SENT_I = -1234.5, -(2 ** 62) + 12345


class Case:
    def __init__(self, dev):
        self.dev = dev
        self.ol = O.OpList()
        self.guards = []            # (buffer, number of payload elements, sentinel value)
        self.outs = {}              # name -> (view, initial copy)
        self.ref = None
        self.t = {}
        self.info = {}

    def operand(self, t):
        """A copy of t on the device between PAD NaN (floating point) / sentinel (integer) elements."""
        n = t.numel()
        if t.is_floating_point():
            buf = torch.full((n + 2 * PAD,), float('nan'), dtype=t.dtype)
        else:
            buf = torch.full((n + 2 * PAD,), 0xFF if t.dtype == torch.uint8 else -12345, dtype=t.dtype)
        buf[PAD:PAD + n] = t.reshape(-1)
        buf = buf.to(self.dev)
        self.ol.keep.append(buf)
        return buf[PAD:PAD + n].view(t.shape)

    def linear(self, w, b):
        return PackedLinear(self.operand(w.to(BF16)), self.operand(b.float()), w.shape[0], w.shape[1])

    def output(self, name, shape, dtype, init=None):
        """An output between sentinel elements; floats start as NaN (an element the launch leaves out fails its bound), accumulators as init."""
        n = 1
        for s in shape:
            n *= s
        sent = SENT_I if dtype == I64 else 0xA5 if dtype == torch.uint8 else -12345 if dtype == torch.int32 else SENT_F
        buf = torch.full((n + 2 * PAD,), sent, dtype=dtype)
        if init is not None:
            buf[PAD:PAD + n] = init.reshape(-1)
        elif dtype.is_floating_point:
            buf[PAD:PAD + n] = float('nan')
        else:
            buf[PAD:PAD + n] = 0
        buf = buf.to(self.dev)
        view = buf[PAD:PAD + n].view(shape)
        self.guards.append((buf, n, sent))
        self.outs[name] = (view, view.clone())
        return view

    def guards_intact(self):
        for buf, n, sent in self.guards:
            if not (bool((buf[:PAD] == sent).all()) and bool((buf[PAD + n:] == sent).all())):
                return False
        return True

    def reset(self):
        for view, init in self.outs.values():
            view.copy_(init)

    def got(self, name):
        view, init = self.outs[name]
        if view.dtype == I64:
            return view.to(torch.float64) / A.QSCALE
        return view.reshape(-1, view.shape[-1])

    def raw(self, name):
        return self.outs[name][0]


def _fin(c, loc):
    c.t = {k: v for k, v in loc.items() if k != 'c'}      # the operands by the builder's own names
    return c


def _rows(g, M, regime):
    v = torch.randn((M, C), generator=g)
    if regime == 'sparse':
        v = (v - 0.45).clamp(min=0) * torch.exp2(torch.rand(C, generator=g) * 12 - 6)
    return v.float()


def _w(g, n, kd, regime, big=False):
    w = torch.randn((n, kd), generator=g) / kd ** 0.5
    if regime == 'large' and big:
        w[::5] *= 16
    return w, torch.randn(n, generator=g) * 0.1


def _ln(g):
    return (torch.rand(C, generator=g) + 0.5).float(), (torch.randn(C, generator=g) * 0.1).float()


def _acc(g, M):
    a = torch.round(torch.randn((M, C), generator=g).double() * 0.3 * A.QSCALE)
    idx = torch.randint(0, M * C, (6,), generator=g)
    a.view(-1)[idx] = torch.tensor([1.0, -1.0, 1.0, -1.0, 1.0, -1.0], dtype=torch.float64) * 2.0 ** 40 + torch.round(torch.randn(6, generator=g).double() * 1e6)
    return a.to(I64)


def pixel_rows(g, K, HW, layout, gap, live):
    """bf16 pixel rows [k | v | q2] (layout 'sep': voff 256, head stride 32) or [k_0 v_0 | k_1 v_1 | .. | q2] ('inter': voff 32, head stride
    64), row stride 768 (+ 8 with gap); the thirds not in `live` ('kv' or 'q') and the gap hold NaN."""
    ld = 3 * C + (8 if gap else 0)
    t = torch.full((K, HW, ld), float('nan'), dtype=BF16)
    if live == 'kv':
        t[..., :2 * C] = torch.randn((K, HW, 2 * C), generator=g).to(BF16)
    else:
        t[..., 2 * C:3 * C] = torch.randn((K, HW, C), generator=g).to(BF16)
    lay = dict(voff=C, hstride=32) if layout == 'sep' else dict(voff=32, hstride=64)
    return t, ld, lay


Q2P_FORMS = ('q_fg', 'q_lg', 'proj', 'chain', 'chain_acc', 'chain_qpre')


def build_q2p(dev, *, K, HW, form, regime='randn', layout='sep', gap=False, Kg=None, n_fg=None, sat=None, seed=0, aux=False):
    """One ATTN_Q2P launch.  form: 'q_fg' (q, mask bytes and counts given), 'q_lg' (q given, mask from the logits), 'proj' (q projected in
    the launch, attention output stored), 'chain' / 'chain_acc' / 'chain_qpre' (output projection into the accumulator; rows with an
    accumulator input; q handed in projected).  aux: an AUX_MASK launch on the same logits in front, its bytes and counts compared exactly."""
    g = torch.Generator().manual_seed(seed)
    c = Case(dev)
    M = K * Q
    chain = form.startswith('chain')
    assert layout == 'sep' or chain
    lg_h = A.mask_logits(g, K, HW, Kg=Kg, sat=sat, n_fg=n_fg)
    fg_h, _ = A.mask_ref64(lg_h, Kg)
    c.info['n_fg'] = fg_h.sum(1)
    kv_h, ldkv, lay = pixel_rows(g, K, HW, layout, gap, 'kv')
    kv = c.operand(kv_h)
    lg = c.operand(lg_h)
    kw = dict(K=K, Q=Q, HW=HW, C=C, heads=HEADS, ldkv=ldkv, voff=lay['voff'])
    rk = dict(K=K, HW=HW, ldkv=ldkv, voff=lay['voff'], hstride=lay['hstride'], Kg=Kg)
    if aux:
        fgo, nfo = c.output('aux_fg', (K, HW), torch.uint8), c.output('aux_nfg', (K,), torch.int32)
        assert Kg in (None, K)
        c.ol.aux_mask(lg, fgo, nfo, K=K, HW=HW)
    qscale = 8.0 if regime == 'large' else 1.0
    if form in ('q_fg', 'q_lg'):
        q = c.operand(torch.randn((M, C), generator=g).float() * qscale)
        y = c.output('y', (M, C), F32)
        if form == 'q_fg':
            fg, nfg = c.operand(fg_h.to(torch.uint8)), c.operand(fg_h.sum(1).to(torch.int32))
            c.ol.attn_q2p(q, kv, fg, nfg, y, **kw)
            c.ref = lambda mut=(): A.q2p_ref64(kv, q=q, fg=fg, nfg=nfg, mut=mut, **rk)
        else:
            c.ol.attn_q2p(q, kv, None, None, y, logits=lg, **kw)
            c.ref = lambda mut=(): A.q2p_ref64(kv, q=q, lg=lg, mut=mut, **rk)
        return _fin(c, locals())
    Wo = c.linear(*_w(g, C, C, regime))
    if form == 'chain_qpre':
        qp = c.operand(torch.randn((M, C), generator=g).float() * (qscale / 32 ** 0.5))
        acc0 = _acc(g, M)
        acc = c.output('acc', (M, C), I64, init=acc0)
        c.ol.attn_q2p(None, kv, None, None, None, logits=lg, q_pre=qp, out_proj=(Wo, acc), hstride=lay['hstride'], clip_objects=Kg, **kw)
        a0 = c.outs['acc'][1]
        c.ref = lambda mut=(): A.q2p_ref64(kv, q_pre=qp, lg=lg, out=dict(Wo=Wo.weight, acc0=a0), mut=mut, **rk)
        return _fin(c, locals())
    x = c.operand(_rows(g, M, regime))
    emb = c.operand(torch.randn((M, C), generator=g).float() * 0.5)
    lg_, lb_ = (c.operand(t) for t in _ln(g))
    Wq = c.linear(*_w(g, C, C, regime, big=True))
    pin = dict(x=x, W=Wq.weight, bias=Wq.bias, emb=emb, ln_g=lg_, ln_b=lb_)
    ln_out = c.output('ln_out', (M, C), F32)
    proj = dict(x=x, W=Wq, emb=emb, ln=(lg_, lb_), ln_out=ln_out)
    if form == 'proj':
        y = c.output('y', (M, C), F32)
        c.ol.attn_q2p(None, kv, None, None, y, logits=lg, proj=proj, **kw)
        c.ref = lambda mut=(): A.q2p_ref64(kv, proj_in=pin, lg=lg, mut=mut, **rk)
        return _fin(c, locals())
    acc_in = None
    if form == 'chain_acc':
        ai, ab = c.operand(_acc(g, M)), c.operand(torch.randn(C, generator=g).float() * 0.1)
        acc_in = (ai, ab)
        pin.update(acc=ai, abias=ab)
    acc = c.output('acc', (M, C), I64, init=_acc(g, M))
    a0 = c.outs['acc'][1]
    c.ol.attn_q2p(None, kv, None, None, None, logits=lg, proj=proj, acc_in=acc_in, out_proj=(Wo, acc), hstride=lay['hstride'], clip_objects=Kg, **kw)
    c.ref = lambda mut=(): A.q2p_ref64(kv, proj_in=pin, lg=lg, out=dict(Wo=Wo.weight, acc0=a0), mut=mut, **rk)
    return _fin(c, locals())


def build_self(dev, *, K, form, regime='randn', seed=0):
    """One ATTN_SELF launch: 'plain' ([q | k | v] rows of stride 3 C + 8 given), 'proj' (projected in the launch), 'chain'."""
    g = torch.Generator().manual_seed(seed)
    c = Case(dev)
    M = K * Q
    if form == 'plain':
        ld = 3 * C + 8
        t = torch.full((M, ld), float('nan'))
        t[:, :3 * C] = torch.randn((M, 3 * C), generator=g) * (2.0 if regime == 'large' else 1.0)
        qkv = c.operand(t)
        y = c.output('y', (M, C), F32)
        c.ol.attn_self(qkv, qkv.view(-1)[2 * C:], y, K=K, Q=Q, C=C, heads=HEADS, ldqk=ld, ldv=ld)
        c.ref = lambda mut=(): A.self_ref64(K=K, qk=qkv, v=qkv.view(-1)[2 * C:], ldqk=ld, ldv=ld, mut=mut)
        return _fin(c, locals())
    x = c.operand(_rows(g, M, regime))
    emb = c.operand(torch.randn((M, C), generator=g).float() * 0.5)
    lg_, lb_ = (c.operand(t) for t in _ln(g))
    W = c.linear(*_w(g, 3 * C, C, regime, big=True))
    pin = dict(x=x, W=W.weight, bias=W.bias, emb=emb, ln_g=lg_, ln_b=lb_)
    ln_out = c.output('ln_out', (M, C), F32)
    proj = dict(x=x, W=W, emb=emb, ln=(lg_, lb_), ln_out=ln_out)
    if form == 'proj':
        y = c.output('y', (M, C), F32)
        c.ol.attn_self(None, None, y, K=K, Q=Q, C=C, heads=HEADS, proj=proj)
        c.ref = lambda mut=(): A.self_ref64(K=K, proj_in=pin, mut=mut)
        return _fin(c, locals())
    Wo = c.linear(*_w(g, C, C, regime))
    ai, ab = c.operand(_acc(g, M)), c.operand(torch.randn(C, generator=g).float() * 0.1)
    pin.update(acc=ai, abias=ab)
    acc = c.output('acc', (M, C), I64, init=_acc(g, M))
    a0 = c.outs['acc'][1]
    c.ol.attn_self(None, None, None, K=K, Q=Q, C=C, heads=HEADS, proj=proj, acc_in=(ai, ab), out_proj=(Wo, acc))
    c.ref = lambda mut=(): A.self_ref64(K=K, proj_in=pin, out=dict(Wo=Wo.weight, acc0=a0), mut=mut)
    return _fin(c, locals())


def build_p2q(dev, *, K, HW, form, next_q=False, regime='randn', gap=False, seed=0):
    """One ATTN_P2Q launch: 'plain' (k | v rows given), 'proj' (projected in the launch), 'chain' (accumulator input, MFMA attention,
    next_q: the extra blocks that project the next block's queries).  The pixels' q is the last third of [k | v | q2] rows."""
    g = torch.Generator().manual_seed(seed)
    c = Case(dev)
    M = K * Q
    px_h, ldq, _ = pixel_rows(g, K, HW, 'sep', gap, 'q')
    px = c.operand(px_h)
    qv = px.view(-1)[2 * C:]
    y = c.output('y', (K, HW, C), BF16)
    kw = dict(K=K, Q=Q, HW=HW, C=C, heads=HEADS, ldq=ldq)
    if form == 'plain':
        t = torch.randn((M, 2 * C), generator=g).float() * (2.0 if regime == 'large' else 1.0)
        kvr = c.operand(t)
        c.ol.attn_p2q(qv, kvr, kvr.view(-1)[C:], y, ldkv=2 * C, **kw)
        c.ref = lambda mut=(): A.p2q_ref64(qv, K=K, HW=HW, ldq=ldq, kq=kvr, vq=kvr.view(-1)[C:], ldkv=2 * C, mut=mut)
        return _fin(c, locals())
    x = c.operand(_rows(g, M, regime))
    emb = c.operand(torch.randn((M, C), generator=g).float() * 0.5)
    W = c.linear(*_w(g, 2 * C, C, regime, big=True))
    pin = dict(x=x, W=W.weight, bias=W.bias, emb=emb)
    if form == 'proj':
        c.ol.attn_p2q(qv, None, None, y, proj=dict(x=x, W=W, emb=emb), **kw)
        c.ref = lambda mut=(): A.p2q_ref64(qv, K=K, HW=HW, ldq=ldq, proj_in=pin, mut=mut)
        return _fin(c, locals())
    ai, ab = c.operand(_acc(g, M)), c.operand(torch.randn(C, generator=g).float() * 0.1)
    pin.update(acc=ai, abias=ab)
    nq = nqr = None
    if next_q:
        ng, nb = (c.operand(t) for t in _ln(g))
        Wn = c.linear(*_w(g, C, C, regime, big=True))
        nq = dict(ln=(ng, nb), W=Wn, q_out=c.output('q_out', (M, C), F32), xn_out=c.output('xn_out', (M, C), F32))
        nqr = dict(ln_g=ng, ln_b=nb, W=Wn.weight, bias=Wn.bias)
    c.ol.attn_p2q(qv, None, None, y, proj=dict(x=x, W=W, emb=emb), acc_in=(ai, ab), next_q=nq, **kw)
    c.ref = lambda mut=(): A.p2q_ref64(qv, K=K, HW=HW, ldq=ldq, proj_in=pin, next_q=nqr, chain=True, mut=mut)
    return _fin(c, locals())


def build_qffn(dev, *, K, hid_slice, regime='randn', seed=0):
    g = torch.Generator().manual_seed(seed)
    c = Case(dev)
    M = K * Q
    x = c.operand(_rows(g, M, regime))
    lg_, lb_ = (c.operand(t) for t in _ln(g))
    W1, W2 = c.linear(*_w(g, FF, C, regime, big=True)), c.linear(*_w(g, C, FF, regime))
    ai, ab = c.operand(_acc(g, M)), c.operand(torch.randn(C, generator=g).float() * 0.1)
    x_out = c.output('x_out', (M, C), F32)
    acc = c.output('acc', (M, C), I64, init=_acc(g, M))
    a0 = c.outs['acc'][1]
    c.ol.qffn(x, x_out, acc, rows=M, ln=(lg_, lb_), W1=W1, W2=W2, acc_in=(ai, ab), hid_slice=hid_slice)
    c.ref = lambda mut=(): A.qffn_ref64(x, ai, ab, lg_, lb_, W1.weight, W1.bias, W2.weight, a0, hid_slice=hid_slice, mut=mut)
    return _fin(c, locals())


def build_qinit(dev, *, K, regime='randn', seed=0):
    """QUERY_INIT with its two linears; 'sparse': areas log-uniform in [2^-12, 2^6], so that the 1e-4 in the denominator matters."""
    g = torch.Generator().manual_seed(seed)
    c = Case(dev)
    M = K * Q
    om = torch.rand((M, C + 1), generator=g) + 0.1
    if regime == 'sparse':
        area = torch.exp2(torch.rand(M, generator=g) * 18 - 12)
        om = torch.cat([_rows(g, M, 'sparse').abs() * area.view(-1, 1), area.view(-1, 1)], 1)
    om = c.operand(om.float())
    Wi, We = c.linear(*_w(g, C, C, regime, big=True)), c.linear(*_w(g, C, C, regime))
    ri, re = c.operand(torch.randn((M, C), generator=g).float()), c.operand(torch.randn((M, C), generator=g).float())
    q, e = c.output('query', (M, C), F32), c.output('query_emb', (M, C), F32)
    c.ol.query_init2(om, q, e, rows=M, w_init=Wi, res_init=ri, w_emb=We, res_emb=re)
    c.ref = lambda mut=(): A.query_init2_ref64(om, Wi.weight, Wi.bias, ri, We.weight, We.bias, re, mut=mut)
    return _fin(c, locals())
