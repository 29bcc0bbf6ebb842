"""tests/ref64.py on the host: the float64 conv reference agrees with torch's float64 conv2d, the interpreter's fp32 result lies inside
its per-element bound, and the bound is tight enough that each fault a conv kernel can plausibly make (a K slice, a tap, a shifted halo,
the neighbouring object's or clip's residual, an unwritten ragged tile) leaves it somewhere."""
import math
import pytest
import torch
import torch.nn.functional as F

import ref64 as R
from cutie_amd import ops as O
from cutie_amd.model.weights import pack_conv
from mock_exec import MockExecutor

BF16 = torch.bfloat16


def _case(c, seed, regime='randn'):
    """Operands of a conv case: dict(B, H, W, C1, [C2], Cout, k, [stride, pad, ldx, res ('plain' | 'bcast' | (f0, gap rows)), act,
    relu_in, out_f32]) -> (ConvGeom, x1, x2, packed weights, w fp32 [Cout, Cin, k, k], bias, residual buffer)."""
    g = torch.Generator().manual_seed(seed)
    B, H, W, C1, Cout, k = c['B'], c['H'], c['W'], c['C1'], c['Cout'], c['k']
    C2 = c.get('C2', 0)
    stride, pad = c.get('stride', 1), c.get('pad', (k - 1) // 2)
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    real1 = c.get('real1', C1)
    w = torch.randn(Cout, real1 + C2, k, k, generator=g) / math.sqrt((real1 + C2) * k * k)
    bias = torch.randn(Cout, generator=g) * 0.1
    pc = pack_conv(w, bias, 'cpu', segs=[(real1, C1)] + ([(C2, C2)] if C2 else []))
    ldx1 = c.get('ldx', C1)
    x1 = R.operand(g, B * H * W, C1, regime=regime, ld=ldx1, fill=float('nan'))
    if real1 < C1:
        x1[:, real1:C1] = 0                                            # the producer's zero-padded channels
    x2 = R.operand(g, B * H * W, C2, regime=regime) if C2 else None
    res, f0, f1 = c.get('res'), 0, 0
    if isinstance(res, tuple):
        f0, f1 = res[0], OH * OW + res[1]
    geo = R.ConvGeom(B=B, H=H, W=W, C1=C1, C2=C2, ldx1=ldx1, ldx2=C2, OH=OH, OW=OW, Cout=Cout, KH=k, KW=k, Kpad=pc.kpad, stride=stride,
                     pad=pad, ldr=Cout, relu_in=c.get('relu_in', False), out_f32=c.get('out_f32', False), res_bcast=res not in (None, 'plain'),
                     act=c.get('act', R.ACT_NONE), f0=f0, f1=f1)
    r = None
    if res is not None:
        r = R.operand(g, geo.res_extent(), Cout, regime='randn', scale=c.get('res_scale', 1.0))
    return geo, x1, x2, pc, w, bias, r


def _torch64(geo, x1, x2, w, bias, r, real1):
    """The same conv through torch's float64 conv2d on NCHW tensors, residual and activation applied per object."""
    x = x1.view(geo.B, geo.H, geo.W, geo.ldx1)[..., :real1].double()
    if geo.C2:
        x = torch.cat([x, x2.view(geo.B, geo.H, geo.W, geo.C2).double()], -1)
    if geo.relu_in:
        x = x.clamp(min=0)
    y = F.conv2d(x.permute(0, 3, 1, 2), w.to(BF16).double(), bias.double(), geo.stride, geo.pad).permute(0, 2, 3, 1)
    if r is not None:
        rr = r.double()
        if not geo.res_bcast:
            y = y + rr.view(geo.B, geo.OH, geo.OW, geo.Cout)
        elif geo.f0:
            for q in range(geo.B // geo.f0):
                y[q * geo.f0:(q + 1) * geo.f0] += rr[q * geo.f1:q * geo.f1 + geo.OHW].view(1, geo.OH, geo.OW, geo.Cout)
        else:
            y = y + rr.view(1, geo.OH, geo.OW, geo.Cout)
    return R._act64(y, geo.act).reshape(geo.M, geo.Cout)


AGREE_CASES = [
    dict(B=2, H=9, W=11, C1=64, C2=64, Cout=40, k=3, relu_in=True),                                # two sources
    dict(B=1, H=10, W=13, C1=48, real1=40, Cout=24, k=3, ldx=56),                                  # ragged Cin (40 real of 48), ldx > C
    dict(B=2, H=13, W=15, C1=32, Cout=48, k=3, stride=2, act=R.ACT_RELU),                          # stride 2
    dict(B=1, H=20, W=22, C1=8, real1=5, Cout=64, k=7, stride=2, pad=3, act=R.ACT_RELU),           # 7x7 pad 3 (the stem's form)
    dict(B=3, H=7, W=9, C1=64, Cout=72, k=1, res='bcast', act=R.ACT_SIGMOID, out_f32=True),        # broadcast residual
    dict(B=6, H=5, W=7, C1=64, Cout=40, k=3, res=(3, 11), act=R.ACT_SQ1, out_f32=True),           # grouped residual: 2 clips x 3 objects
    dict(B=2, H=6, W=8, C1=64, Cout=16, k=3, res='plain'),
]


@pytest.mark.parametrize('ci', range(len(AGREE_CASES)))
def test_ref64_matches_torch_float64_conv(ci):
    c = AGREE_CASES[ci]
    geo, x1, x2, pc, w, bias, r = _case(c, seed=ci)
    y64, bound = R.conv_ref64(geo, x1, pc.weight, x2=x2, bias=pc.bias, res=r)
    want = _torch64(geo, x1, x2, w, bias, r, c.get('real1', c['C1']))
    assert torch.isfinite(y64).all() and torch.isfinite(bound).all() and bool((bound > 0).all())
    assert float((y64 - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    rows = R.sample_rows(geo, bm=32, n_random=17, seed=ci)                 # a row subset: the same values
    y64s, bounds = R.conv_ref64(geo, x1, pc.weight, x2=x2, bias=pc.bias, res=r, rows=rows)
    assert torch.equal(y64s, y64[rows]) and torch.equal(bounds, bound[rows])


def _mock(geo, x1, x2, pc, r):
    """The interpreter's result of the same descriptor (fp32 conv on the host, output rounded to the stored format)."""
    y = torch.full((geo.M, geo.ldy), float('nan'), dtype=torch.float32 if geo.out_f32 else BF16)
    ol = O.OpList()
    ol.conv(x1, pc, y, B=geo.B, H=geo.H, W=geo.W, C1=geo.C1, ldx1=geo.ldx1, OH=geo.OH, OW=geo.OW, ldy=geo.ldy, stride=geo.stride, pad=geo.pad,
            x2=x2, C2=geo.C2, ldx2=geo.ldx2, res=r, ldr=geo.ldr, res_bcast=geo.res_bcast, relu_in=geo.relu_in, act=geo.act,
            out_f32=geo.out_f32, tile=2, res_group=(geo.f0, geo.f1) if geo.f0 else None)
    MockExecutor().run(ol.finalize())
    return y[:, :geo.Cout].double()


SOUND_CASES = AGREE_CASES + [
    dict(B=1, H=12, W=14, C1=1024, Cout=256, k=1),                                                  # long K (pix_feat_proj)
    dict(B=3, H=8, W=9, C1=256, Cout=256, k=3, relu_in=True, act=R.ACT_RELU),                      # CAResBlock conv, Kpad 2304
    dict(B=2, H=8, W=9, C1=576, Cout=64, k=3, act=R.ACT_SIGMOID, out_f32=True),                    # Kpad 5248: n u > 2^-12
    dict(B=1, H=6, W=7, C1=256, Cout=2304, k=1, res='plain', res_scale=64.0),                      # large residual, wide Cout
]


@pytest.mark.parametrize('regime', ['randn', 'sparse'])
@pytest.mark.parametrize('ci', range(len(SOUND_CASES)))
def test_ref64_bound_holds_for_the_interpreter(ci, regime):
    """The bound is sound: the interpreter's fp32 conv (another summation order) lies inside it at every element."""
    c = SOUND_CASES[ci]
    geo, x1, x2, pc, w, bias, r = _case(c, seed=50 + ci, regime=regime)
    y64, bound = R.conv_ref64(geo, x1, pc.weight, x2=x2, bias=pc.bias, res=r)
    R.check_bound(_mock(geo, x1, x2, pc, r), y64, bound, f'mock case {ci}')


def _exceeds(geo, y64, bound, y_mut):
    return int(((y_mut - y64).abs() > bound).sum())


# representative production geometries: CAResBlock 3x3 at 480p (3 objects), the 1024 -> 256 1x1 projection, the decoder 3x3 at stride 4
# on 1080p (a row subset), the fusion 1x1 of 4 clips x 3 objects with grouped residual
PROD = dict(
    ca=dict(B=3, H=30, W=54, C1=256, Cout=256, k=3, relu_in=True, act=R.ACT_RELU),
    proj=dict(B=1, H=30, W=54, C1=1024, Cout=256, k=1),
    dec=dict(B=5, H=272, W=480, C1=128, Cout=128, k=3, relu_in=True, act=R.ACT_RELU),
    grp=dict(B=12, H=30, W=54, C1=256, Cout=256, k=1, res=(3, 3 * 30 * 54), act=R.ACT_RELU),
)


def _rows(geo, name):
    return R.sample_rows(geo, bm=128, n_random=1024, seed=3) if name == 'dec' else None


@pytest.mark.parametrize('regime', ['randn', 'sparse'])
@pytest.mark.parametrize('name', ['ca', 'proj', 'dec', 'grp'])
def test_ref64_bound_catches_a_dropped_k_slice(name, regime):
    geo, x1, x2, pc, w, bias, r = _case(PROD[name], seed=7, regime=regime)
    rows = _rows(geo, name)
    y64, bound = R.conv_ref64(geo, x1, pc.weight, x2=x2, bias=pc.bias, res=r, rows=rows)
    K = geo.KH * geo.KW * geo.Cin
    for k0 in (0, K // 2 // 64 * 64, K - 64):                           # first, middle and last 64-channel K slice
        wm = pc.weight.clone()
        wm[:, k0:k0 + 64] = 0
        ym, _ = R.conv_ref64(geo, x1, wm, x2=x2, bias=pc.bias, res=r, rows=rows)
        assert _exceeds(geo, y64, bound, ym) > 0, (name, regime, k0)


@pytest.mark.parametrize('name', ['ca', 'dec'])
def test_ref64_bound_catches_a_dropped_tap(name):
    geo, x1, x2, pc, w, bias, r = _case(PROD[name], seed=8)
    rows = _rows(geo, name)
    y64, bound = R.conv_ref64(geo, x1, pc.weight, x2=x2, bias=pc.bias, res=r, rows=rows)
    for tap in range(9):
        wm = pc.weight.clone()
        wm[:, tap * geo.Cin:(tap + 1) * geo.Cin] = 0
        ym, _ = R.conv_ref64(geo, x1, wm, x2=x2, bias=pc.bias, res=r, rows=rows)
        assert _exceeds(geo, y64, bound, ym) > 0, (name, tap)


@pytest.mark.parametrize('name', ['ca', 'dec'])
@pytest.mark.parametrize('axis', [1, 2])
def test_ref64_bound_catches_a_halo_shifted_by_one_pixel(name, axis):
    geo, x1, x2, pc, w, bias, r = _case(PROD[name], seed=9)
    rows = _rows(geo, name)
    y64, bound = R.conv_ref64(geo, x1, pc.weight, x2=x2, bias=pc.bias, res=r, rows=rows)
    x = x1.view(geo.B, geo.H, geo.W, geo.ldx1)
    xs = torch.zeros_like(x)                                              # the input window read one pixel down / right
    if axis == 1:
        xs[:, :-1] = x[:, 1:]
    else:
        xs[:, :, :-1] = x[:, :, 1:]
    ym, _ = R.conv_ref64(geo, xs, pc.weight, x2=x2, bias=pc.bias, res=r, rows=rows)
    n = _exceeds(geo, y64, bound, ym)
    assert n > 0.5 * y64.numel(), (name, axis, n, y64.numel())


@pytest.mark.parametrize('form', ['plain', 'grouped'])
def test_ref64_bound_catches_the_neighbours_residual_row(form):
    """A residual addressed with the neighbouring object's (plain residual) or the neighbouring clip's (grouped: F_RES_BCAST, f0 > 0) rows."""
    c = dict(PROD['grp'], res='plain', B=3) if form == 'plain' else PROD['grp']
    geo, x1, x2, pc, w, bias, r = _case(c, seed=10, regime='sparse')
    y64, bound = R.conv_ref64(geo, x1, pc.weight, x2=x2, bias=pc.bias, res=r)
    if form == 'plain':
        rm = r.view(geo.B, geo.OHW, geo.Cout).roll(1, 0).reshape(-1, geo.Cout)
    else:
        G = geo.B // geo.f0
        rm = r.clone()
        for q in range(G):                                                 # clip q reads clip q + 1's map
            nq = (q + 1) % G
            rm[q * geo.f1:q * geo.f1 + geo.OHW] = r[nq * geo.f1:nq * geo.f1 + geo.OHW]
    ym, _ = R.conv_ref64(geo, x1, pc.weight, x2=x2, bias=pc.bias, res=rm)
    assert _exceeds(geo, y64, bound, ym) > 0.5 * y64.numel()


@pytest.mark.parametrize('bm', [64, 96, 128, 320])
def test_ref64_bound_catches_an_unwritten_ragged_tile(bm):
    """The last, partial BM-row tile left unwritten (output buffer zero there)."""
    geo, x1, x2, pc, w, bias, r = _case(PROD['ca'], seed=11)
    assert geo.M % bm
    y64, bound = R.conv_ref64(geo, x1, pc.weight, x2=x2, bias=pc.bias, res=r)
    ym = y64.clone()
    ym[(geo.M // bm) * bm:] = 0
    n = _exceeds(geo, y64, bound, ym)
    assert n > 0.2 * (geo.M % bm) * geo.Cout, (bm, n)


def test_sample_rows_cover_borders_tiles_and_patches():
    geo = R.ConvGeom(B=2, H=13, W=17, C1=64, OH=13, OW=17, Cout=8, KH=3, KW=3, Kpad=640, pad=1)
    rows = R.sample_rows(geo, bm=96, halo=(8, 16), n_random=0)
    s = set(rows.tolist())
    M = geo.M
    assert all(m in s for m in range(M - M % 96, M))                       # last ragged tile
    assert all(m in s for q in range(96, M, 96) for m in (q - 1, q))       # both sides of every tile boundary
    for b in range(2):
        for oh in range(13):
            for ow in range(17):
                m = (b * 13 + oh) * 17 + ow
                if oh in (0, 12, 7, 8) or ow in (0, 16, 15):
                    assert m in s, (b, oh, ow)
    assert rows.tolist() == sorted(s)


def test_gap_fixed_point_formula():
    """The GAP side job's per-value fixed point (conv_common.h conv_gapfx): exact through 2^20, saturating beyond, NaN = 0."""
    v = torch.tensor([0.0, 2.0 ** -21, 3 * 2.0 ** -21, -2.0 ** -21, 1.5, 2047.0, 2048.0, 2.0 ** 20, 2.0 ** 20 + 2 ** 13, -3e6,
                      float('inf'), float('-inf'), float('nan'), 123456.0])
    want = [0, 0, 2, 0, 1572864, 2047 << 20, 2048 << 20, 1 << 40, 1 << 40, -(1 << 40), 1 << 40, -(1 << 40), 0, 123456 << 20]
    assert R.gap_fixed(v).tolist() == want
