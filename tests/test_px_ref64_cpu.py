"""tests/px_ref64.py on the host: the float64 functions are the reference algorithm (oracle.net's aggregate, _gru, _others and _ca_block
arithmetic, torch.nn.functional's bilinear / area interpolation, pooling and softmax, all run in float64); the interpreter's fp32 results
(tests/mock_exec.py) lie inside every bound and pass every exact check, for every case of the list that tests/test_gpu_px_ref64.py runs
on the kernels; no case yields a non-finite reference or bound; and the checks bite: each fault a pixel kernel can plausibly make, applied
to the outputs of a case, crosses a bound or an exact check in at least one case of the shared list -- or is listed in INVISIBLE with the
reason why no bound can see it (DESIGN.md keeps the table)."""
import math

import pytest
import torch
import torch.nn.functional as F

import px_ref64 as P
from mock_exec import MockExecutor
from oracle import net as oracle_net

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def launch(ol):
    arr = ol.finalize()
    run = lambda: MockExecutor().run(arr)
    run()
    return run


def close(a, b, rel=1e-11):
    scale = max(1.0, float(b.abs().max()))
    return float((a - b).abs().max()) <= rel * scale


# ---- the float64 functions are the reference algorithm -----------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', [0.5, 0.25])
def test_bilinear_is_torch_interpolate_and_its_weights_are_exact_dyadics(scale):
    g = P.gen(1)
    for h, w in ((1, 1), (1, 9), (7, 1), (2, 2), (3, 5), (7, 9), (12, 20)):
        a = torch.randn((3, h, w), generator=g, dtype=F64)
        v, _, _ = P.bilinear_ref(a, 0, scale)
        want = F.interpolate(a[None], scale_factor=1 / scale, mode='bilinear', align_corners=False)[0]
        assert close(v, want)
        *_, W = P.bilinear_weights(h, w, scale)
        unit = 2.0 ** (-4 if scale == 0.5 else -6)
        for wt in W:
            assert torch.equal(wt.to(F32).to(F64), wt) and bool(((wt / unit) == (wt / unit).round()).all()) and bool(((wt >= 0) & (wt <= 1)).all())
        assert close(sum(W), torch.ones_like(W[0]), 0)


def test_area_pool_maxpool_and_means_are_torch_functional():
    g = P.gen(2)
    for r in (2, 3, 4, 8):
        x = torch.randn((2, 3 * r, 5 * r, 8), generator=g, dtype=F64)
        want = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=1 / r, mode='area').permute(0, 2, 3, 1)
        assert close(P.area_down_ref(x, r)['y'][0], want)
    for H, W in ((1, 1), (7, 9), (8, 8)):
        x = P.bf16_map(g, (2, H, W, 8), 'plain')
        want = F.max_pool2d(x.double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
        assert torch.equal(P.maxpool_ref(x, False)['y'][0], want) and torch.equal(P.maxpool_ref(x, True)['y'][0], want.clamp(min=0))
    m = torch.rand((4, 32, 48), generator=g, dtype=F64)
    ref = P.mask_down_ref(m)
    m16 = F.avg_pool2d(m[None], 16)[0]
    assert close(ref['m16'][0], m16)
    others = oracle_net.OracleNet._others(m16[None])[0]
    assert close(ref['pair'][0][..., 1], others) and close(ref['pair'][0][..., 0], m16)
    x = torch.randn((2, 513, 64), generator=g).to(BF16)
    assert close(P.gap_ref(x)['y'][0], x.double().mean(1))


def test_img_prep_others_is_the_oracles():
    g = P.gen(3)
    masks = torch.rand((3, 32, 48), generator=g)
    img = torch.rand((3, 30, 43), generator=g)
    y = P.img_prep_ref(img, masks, P.IMG_MEAN, P.IMG_STD, H=32, W=48, pl=2, pt=1)['y'][0]
    assert close(y[..., 4], oracle_net.OracleNet._others(masks.double()[None])[0])
    full = F.pad(img.double(), (2, 3, 1, 1))
    mean, std = torch.tensor(P.IMG_MEAN, dtype=F32).double().view(3, 1, 1), torch.tensor(P.IMG_STD, dtype=F32).double().view(3, 1, 1)
    assert close(y[0, ..., :3], ((full - mean) / std).permute(1, 2, 0))


def test_gru_is_the_oracles():
    g = P.gen(4)
    v, h = P.gru_inputs(g, 5, 64, 'plain')
    want = oracle_net.OracleNet._gru(h.double()[None], v.double()[None])[0]
    assert close(P.gru_ref(v, h)['h'][0], want)


def test_eca_is_the_ca_block_arithmetic():
    g = P.gen(5)
    B, HW, C = 2, 65, 64
    x, r, wk = P.bf16_map(g, (B, HW, C), 'plain'), P.bf16_map(g, (B, HW, C), 'plain'), torch.randn(5, generator=g)
    part = P.gap_ref(x)['part'][0]
    ref = P.eca_apply_ref(x, r, wk, part=part)
    x64 = x.double().permute(0, 2, 1).reshape(B, C, HW, 1)
    w = x64.mean(dim=(2, 3)).view(B, 1, C)                                # oracle.net.OracleNet._ca_block, from its mean on
    w = F.conv1d(w, wk.double().view(1, 1, 5), None, 1, 2).transpose(-1, -2).unsqueeze(-1).sigmoid()
    want = (x64 * w + r.double().permute(0, 2, 1).reshape(B, C, HW, 1))[..., 0].permute(0, 2, 1)
    assert close(ref['y'][0], want)
    fixed = P.gap_fixed(x.float()).sum(1) * 16
    assert close(P.eca_apply_ref(x, r, wk, fixed=fixed)['y'][0], want, 1e-6)          # (the fixed point itself: 2^-21 of the mean)
    pw, pb = (torch.randn(256, generator=g) / 8).to(BF16), torch.randn(1, generator=g)
    y = torch.randn((1, 7, 256), generator=g).to(BF16)
    head = P.eca_head_ref(pw, pb, stored=y)['plog'][0]
    assert close(head, F.conv2d(F.relu(y.double()).permute(0, 2, 1)[..., None], pw.double().view(1, 256, 1, 1), pb.double())[:, 0, :, 0])


def test_seg_tail_is_aggregate_bilinear_softmax(monkeypatch):
    """oracle.net.aggregate casts to fp32 first; with that cast switched off it runs in float64.  Logits within +-12 keep every plane off the
    clamps, where aggregate's float64 clamp constants and the kernels' fp32 ones would differ (shown apart below)."""
    g = P.gen(6)
    x = (torch.rand((3, 5, 7), generator=g, dtype=F64) * 2 - 1) * 5
    monkeypatch.setattr(torch.Tensor, 'float', lambda self: self)
    want = oracle_net.aggregate(torch.sigmoid(x), 0)
    monkeypatch.undo()
    assert want.dtype == F64
    a, _ = P.agg_ref(x)
    assert close(a, want)
    ref = P.up4_fused_ref(x)
    up = F.interpolate(want[None], scale_factor=4, mode='bilinear', align_corners=False)[0]
    assert close(ref['lup'][0], up) and close(ref['prob'][0], F.softmax(up, 0))
    planes = torch.rand((4, 257), generator=g, dtype=F64) * 0.4
    monkeypatch.setattr(torch.Tensor, 'float', lambda self: self)
    want = F.softmax(oracle_net.aggregate(planes, 0), 0)
    monkeypatch.undo()
    assert close(P.agg_softmax_ref(planes)['prob'][0], want)


def test_the_clamp_constants_are_the_fp32_ones():
    """On fp32 tensors -- what the model runs -- aggregate's clamp(1e-7, 1 - 1e-7) uses float32(1e-7) and float32(1 - 1e-7) = 1 - 2^-23: a saturated
    plane is logit(1 - 2^-23) = 15.94, not logit(1 - 1e-7) = 16.12, and the reference says so within its bound."""
    assert P.HI32 == 1 - 2.0 ** -23 and abs(P.LO32 - 1e-7) < 1e-14 and P.LO32 != 1e-7
    sat = oracle_net.aggregate(torch.tensor([[1.0, 0.0]]), 0)
    hi, lo = float(P.logit64(torch.tensor(P.HI32, dtype=F64))), float(P.logit64(torch.tensor(P.LO32, dtype=F64)))
    assert abs(hi - 15.9424) < 1e-3 and abs(hi - math.log((1 - 1e-7) / 1e-7)) > 0.1
    y, e = P.clamp_logit_ref(torch.tensor([1.0, 0.0, 1 - 1e-9, 1e-9], dtype=F64), 0.0)
    assert close(y, torch.tensor([hi, lo, hi, lo], dtype=F64)) and float(e.max()) < 1e-5
    assert bool(((sat[1].double() - torch.tensor([hi, lo])).abs() <= e[:2]).all())
    # next to a clamp either side is legal: the hull reaches from the unclamped value to the constant
    y, e = P.clamp_logit_ref(torch.tensor([P.HI32 - 2.0 ** -24], dtype=F64), 2.0 ** -24)
    assert float(y + e) >= hi and float(y - e) <= float(P.logit64(torch.tensor(P.HI32 - 2.0 ** -23, dtype=F64)))


def test_the_clamp_logit_bound_widths_the_docstring_states():
    for logit, want in ((6.0, 4.8e-5), (12.0, 2.0e-2), (16.0, 0.66)):
        p = torch.sigmoid(torch.tensor([logit], dtype=F64))
        _, e = P.clamp_logit_ref(p, 2 * P.U32)
        assert abs(float(e) / want - 1) < 0.1, (logit, float(e))


def test_on_the_clamps_the_bound_is_that_of_logf_of_two_constants():
    """|x| = 25, where real frames sit: the sigmoid rounds to 1.0f or to e^-25, bg to a product beyond the clamp, and every plane -- object,
    background, with one, no or two objects saturated, and mixed with |x| = 18 .. 20 -- is a constant within LOG_ULP ulp of itself plus the 2 u of
    the ratio; the fused probabilities from the raw logits are then within 1e-5, the dominant one and the negligible ones alike."""
    top = float(P.logit64(torch.tensor(P.HI32, dtype=F64)))
    ulp3 = P.LOG_ULP * 2.0 ** -23 * 16.2 + 3 * P.U32
    for pat in ([25.0, -25.0, -25.0], [-25.0, -25.0, -25.0], [25.0, 25.0, -25.0], [18.0, -20.0, -25.0], [-18.0], [19.0]):
        x = torch.tensor(pat, dtype=F64).view(-1, 1, 1).expand(-1, 4, 4).contiguous()
        a, e = P.agg_ref(x)
        assert bool(((a.abs() - top).abs() < 0.2).all()) and float(e.max()) <= ulp3, (pat, float(e.max()))
        ref = P.up4_fused_ref(x, mask_down=True)
        assert float(ref['lup'][1].max()) <= 2e-5 and float(ref['prob'][1].max()) <= 1e-5 and float(ref['m16'][1].max()) <= 4e-5, pat
        w, b = ref['prob']
        assert bool((b[w < 1e-6] <= 1e-5 * w[w < 1e-6] + 1e-15).all())          # a negligible plane: relative to its own weight
    # the large regime of the shared cases: the bound of a dominant probability is 1e-5 on all but the transition pixels
    x = P.seg_logits(P.gen(0), 3, 12, 20, 'large')
    w, b = P.up4_fused_ref(x)['prob']
    assert float(b[w > 0.5].median()) <= 1e-5 and float((b[w > 0.5] > 1e-2).float().mean()) < 0.05
    # from the stored aggregate (the two-launch form) every probability is within 1e-5, transitions included
    a, _ = P.agg_ref(x)
    assert float(P.up4_softmax_ref(a.float())['prob'][1].max()) <= 1e-5


# ---- the interpreter is inside every bound (and no case yields a non-finite reference: the runners assert all_finite) -------------------
@pytest.mark.parametrize('case', P.ALL_CASES, ids=P.case_id)
def test_the_interpreter_lies_inside_every_bound(case):
    op, kw = case
    ratios = P.RUNNERS[op][0]('cpu', launch, **kw)
    assert max(ratios.values()) <= 1.0


def test_the_case_list_holds_what_the_kernels_can_get_wrong():
    up4 = P.UP4_CASES
    assert {c['K'] for c in up4} == {1, 2, 3, 4, 5, 6, 7, 8, 15} and {(c['h'], c['w']) for c in up4 if c['K'] == 3} == set(P.UP4_SIZES)
    assert {c['HW'] for c in P.GAP_CASES} == set(P.GAP_HW) and {c['C'] for c in P.GAP_CASES} == {8, 32, 64, 128, 256}
    assert {(c['n'], c['C']) for c in P.GRU_CASES} >= {(1, 4), (3, 64), (5, 256), (257, 8), (7, 6)}
    assert {c['counts'] for c in P.CLIP_CASES} == {(2, 2), (3, 3, 3), (1, 3), (3, 1), (7, 1, 2), (2, 2, 2)}
    assert {c['r'] for c in P.AREA_CASES} == {2, 3, 4, 8} and {c['hw'] for c in P.PLAIN_CASES} == {1, 255, 256, 257}
    g = P.gen(0)
    x = P.seg_logits(g, 3, 12, 20, 'large')                                # the large regime holds every pixel class
    a, _ = P.agg_ref(x)
    top, bot = float(P.logit64(torch.tensor(P.HI32, dtype=F64))), float(P.logit64(torch.tensor(P.LO32, dtype=F64)))
    on_clamp = (a == top) | (a == bot)
    assert bool(on_clamp.all(0).any()) and bool((~on_clamp).any()) and float((x.abs() > 17).float().mean()) > 0.5
    assert bool(((a[1:] == top).sum(0) == 1).any())


# ---- the checks bite ---------------------------------------------------------------------------------------------------------------------
def _coords(n_out, n_in, s, mut):
    src = ((torch.arange(n_out, dtype=F64) + 0.5) * s - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1) % n_in if mut == 'i1_not_clamped' else (i0 + 1).clamp(max=n_in - 1)
    return i0, i1, src - i0.to(F64)


def _bil(a, scale, mut=None):
    h, w = a.shape[-2:]
    OH, OW = int(round(h / scale)), int(round(w / scale))
    s = 0.5 if mut == 'scale_half' else scale
    y0, y1, ly = _coords(OH, h, s, mut)
    x0, x1, lx = _coords(OW, w, s, mut)
    ly, lx = ly.view(-1, 1), lx.view(1, -1)
    W = [(1 - ly) * (1 - lx), (1 - ly) * lx, ly * (1 - lx), ly * lx]
    if mut == 'lx_ly_swapped':
        W[1], W[2] = W[2], W[1]
    t = lambda yy, xx: a[..., yy, :][..., :, xx]
    return W[0] * t(y0, x0) + W[1] * t(y0, x1) + W[2] * t(y1, x0) + W[3] * t(y1, x1)


def _agg(x, mut=None):
    p = torch.sigmoid(x.double())
    lo, hi = (1e-6, 1 - 1e-6) if mut == 'clamp_1e-6' else (P.LO32, P.HI32)
    cl = lambda q: torch.log(q.clamp(lo, hi) / (1 - q.clamp(lo, hi)))
    q = 1 - p
    if mut == 'bg_without_one_object' and x.shape[0] > 1:
        q = q[:-1]
    if mut == 'clamp_before_product':
        bg = q.clamp(lo, hi).prod(0)
        l0 = torch.log(bg / (1 - bg))
    else:
        l0 = cl(q.prod(0))
    return torch.cat([l0[None], cl(p)])


def _softmax(v, mut=None):
    if mut == 'softmax_without_max':
        e = torch.exp(v.float())                                            # fp32, as the kernel would
        return (e / e.sum(0, keepdim=True)).double()
    return F.softmax(v, 0)


def _mut_up4(mut):
    def f(c):
        a = _agg(c.x, mut)
        v = _bil(a, 0.25, mut)
        prob = _softmax(v, mut)
        c.agg.copy_(a)
        for p, l in [(c.two_p, c.two_l)] + [(o[0], o[1]) for o in c.outs.values()]:
            p.copy_(prob)
            if l is not None:
                l.copy_(v)
        if not c.sep:
            return
        md = P.mask_down_ref(prob[1:])                                      # what follows from the probabilities follows from the mutated ones
        for m16, pair, _ in [o[2] for o in c.outs.values() if o[2]] + [c.sep + (64,)]:
            m16.copy_(md['m16'][0])
            pair[..., :8].copy_(md['pair'][0])
    return f


def _mut_agg_softmax(mut):
    def f(c):
        p = c.planes.double()
        lo, hi = (1e-6, 1 - 1e-6) if mut == 'clamp_1e-6' else (P.LO32, P.HI32)
        cl = lambda q: torch.log(q.clamp(lo, hi) / (1 - q.clamp(lo, hi)))
        q = (1 - p)[:-1] if mut == 'bg_without_one_object' and c.K > 1 else 1 - p
        if mut == 'clamp_before_product':
            bg = q.clamp(lo, hi).prod(0)
            l0 = torch.log(bg / (1 - bg))
        else:
            l0 = cl(q.prod(0))
        c.prob.copy_(_softmax(torch.cat([l0[None], cl(p)]), mut).view(c.prob.shape))
    return f


def _mut_clips(mut):
    def f(c):
        for i, k in enumerate(c.counts):
            early = 1 if mut == 'planes_one_early' and i > 0 else 0          # the clip's planes started one plane early
            ref = P.up4_fused_ref(c.x[c.st[i] - early:c.st[i] - early + k], mask_down=bool(c.h % 4 == 0 and c.w % 4 == 0))
            o = c.st[i] + i
            for prob, lup, m16, pair in c.outs.values():
                prob[o:o + k + 1].copy_(ref['prob'][0])
                lup[o:o + k + 1].copy_(ref['lup'][0])
                if not bool(torch.isnan(m16).all()):
                    m16[c.st[i]:c.st[i] + k].copy_(ref['m16'][0].reshape(k, -1))
                    pair[c.st[i]:c.st[i] + k].copy_(ref['pair'][0].reshape(k, -1, 8))
    return f


def _mut_upsample(mut):
    def f(c):
        nmap = max(c.grp) + 1
        grp = [(q + 1) % nmap for q in c.grp] if mut == 'skip_from_wrong_group' else c.grp
        C = c.x.shape[-1]
        v = _bil(c.x.double().permute(0, 3, 1, 2), 0.5, mut).permute(0, 2, 3, 1)
        sk = torch.stack([c.skip[q, :4 * c.h * c.w].view(2 * c.h, 2 * c.w, C).double() for q in grp])
        for y in c.ys:
            y.copy_(v + sk)
    return f


def _mut_gru(mut):
    def f(c):
        v, h, C = c.v.double(), c.h0.double(), c.C
        fg, u, n = torch.sigmoid(v[:, :C]), torch.sigmoid(v[:, C:2 * C]), torch.tanh(v[:, 2 * C:])
        if mut == 'u_f_swapped':
            fg, u = u, fg
        if mut == 'tanh_is_sigmoid':
            n = torch.sigmoid(v[:, 2 * C:])
        y = fg * h * (1 - u) + u * n
        for h, hb in c.outs.values():
            h.copy_(y)
            hb.copy_(y.view(hb.shape))
    return f


def _mut_mask_down(mut):
    def f(c):
        K, H, W = c.m.shape
        s = c.m.double().reshape(K, H // 16, 16, W // 16, 16).sum((2, 4))
        a = s / (255 if mut == 'mean_over_255' else 256)
        o = a.sum(0, keepdim=True) - a
        o = o if mut == 'others_not_clamped' else o.clamp(0, 1)
        c.m16.copy_(a)
        c.pair[..., 0].copy_(a)
        c.pair[..., 1].copy_(o)
    return f


def _mut_img_prep(mut):
    def f(c):
        if c.masks is not None:
            m = c.masks.double()
            o = m.sum(0, keepdim=True) - m
            c.y[..., 4].copy_(o if mut == 'others_not_clamped' or c.K == 1 else o.clamp(0, 1))
    return f


def _mut_area(mut):
    def f(c):
        t = c.xb.double()
        B, H, W, C = t.shape
        r = c.r
        oh, ow = H // r, W // r
        y = t[:, :oh * r, :ow * r].reshape(B, oh, r, ow, r, C).sum((2, 4)) / (r if mut == 'mean_with_r' else r * r)
        for cat in c.cats.values():
            cat[..., C:2 * C].copy_(y)
    return f


def _mut_eca(mut):
    def f(c):
        x, r, wk = c.x.double(), c.res.double(), c.wk.double()
        C = c.C
        mean = x.mean(1)
        taps = wk.flip(0) if mut == 'taps_reversed' else wk
        if mut == 'padding_wraps':
            mp = torch.cat([mean[:, -2:], mean, mean[:, :2]], 1)
        else:
            mp = F.pad(mean, (2, 2))
        s = torch.sigmoid(sum(taps[j] * mp[:, j:j + C] for j in range(5)))
        y = x * s[:, None] + r
        for name, (src, yo, gout, plog, head) in c.forms.items():
            if mut in ('taps_reversed', 'padding_wraps'):
                yo.copy_(y)
            if head:
                src_y = y if mut == 'head_reads_unrounded_y' else yo.double()
                act = src_y if mut == 'head_without_relu' else src_y.clamp(min=0)
                plog.copy_((act * c.pw.double()).sum(-1) + (float(c.pb) if head == 'bias' else 0.0))
    return f


# (op, mutation, how): every one must fail a bound or an exact check in at least one case of the op's shared list
MUTATIONS = [
    ('up4', 'i1_not_clamped', _mut_up4), ('up4', 'lx_ly_swapped', _mut_up4), ('up4', 'scale_half', _mut_up4),
    ('up4', 'bg_without_one_object', _mut_up4), ('up4', 'clamp_before_product', _mut_up4), ('up4', 'clamp_1e-6', _mut_up4),
    ('merge_agg', 'bg_without_one_object', _mut_agg_softmax), ('merge_agg', 'clamp_before_product', _mut_agg_softmax), ('merge_agg', 'clamp_1e-6', _mut_agg_softmax),
    ('upsample', 'i1_not_clamped', _mut_upsample), ('upsample', 'lx_ly_swapped', _mut_upsample), ('upsample', 'skip_from_wrong_group', _mut_upsample),
    ('gru', 'u_f_swapped', _mut_gru), ('gru', 'tanh_is_sigmoid', _mut_gru),
    ('mask_down', 'mean_over_255', _mut_mask_down), ('mask_down', 'others_not_clamped', _mut_mask_down),
    ('img_prep', 'others_not_clamped', _mut_img_prep),
    ('gap_eca', 'taps_reversed', _mut_eca), ('gap_eca', 'padding_wraps', _mut_eca), ('gap_eca', 'head_reads_unrounded_y', _mut_eca),
    ('gap_eca', 'head_without_relu', _mut_eca),
    ('area', 'mean_with_r', _mut_area),
    ('up4_clips', 'planes_one_early', _mut_clips),
]
# what no bound can see, and why
INVISIBLE = {
    'softmax_without_max': 'every logit into a softmax of the seg tail went through clamp_logit: |v| <= logit(1 - 2^-23) = 15.95, so exp(v) <= 8.4e6 and a sum '
                           'of 17 planes stays far below the fp32 range; without the subtraction the result differs by roundings the bound already holds',
    'i0_clamped_for_rows_only': 'src <= n - 5/8 for every output index, so floor(src) <= n - 1 and the clamp of i0 never acts, for rows or columns',
}


def _caught_by(op, mutate):
    """The first case of the op's list in which the mutated outputs fail a check; None when every case passes."""
    run, cases = P.RUNNERS[op]
    for kw in cases:
        try:
            run('cpu', launch, mutate=mutate, **kw)
        except AssertionError as e:
            return kw, str(e)
    return None


@pytest.mark.parametrize('op,mut,make', MUTATIONS, ids=[f'{m[0]}-{m[1]}' for m in MUTATIONS])
def test_the_checks_bite(op, mut, make):
    hit = _caught_by(op, make(mut))
    assert hit is not None, f'{mut} passes every {op} case'
    assert 'float64 bound' in hit[1], (mut, 'failed something else than a bound or an exact check', hit[1][:200])


CONTROLS = sorted({(m[0], m[2]) for m in MUTATIONS}, key=lambda t: (t[0], t[1].__name__))


@pytest.mark.parametrize('op,make', CONTROLS, ids=[f'{c[0]}-{c[1].__name__}' for c in CONTROLS])
def test_the_unmutated_restatement_passes_every_case(op, make):
    """The control of test_the_checks_bite: the same float64 restatement with no fault in it, written over the outputs, passes every case --
    so a fault that is caught is caught for the fault, not for a slip in the restatement."""
    assert _caught_by(op, make(None)) is None


@pytest.mark.parametrize('op,make', [('up4', _mut_up4), ('merge_agg', _mut_agg_softmax)])
def test_what_the_bound_provably_cannot_see(op, make):
    assert _caught_by(op, make('softmax_without_max')) is None
    for n in (1, 2, 3, 7, 12, 20):                                          # the clamp of i0 is dead code at both scales
        for s in (0.5, 0.25):
            src = ((torch.arange(int(n / s), dtype=F64) + 0.5) * s - 0.5).clamp(min=0)
            assert int(src.floor().max()) <= n - 1
