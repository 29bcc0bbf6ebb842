"""Lock step for clips with DIFFERENT object counts on the MI355X: a mixed group through LockstepCores(mixed_objects=True) against every
clip's own InferenceCore run, bit for bit (the assertions of test_gpu_parity.py::test_lockstep_clips_match_sequential); and every mixed
form of the descriptors (include/cutie_hip.h: UPSAMPLE2X_ADD i6, COPY2D i4, UP4_SOFTMAX i5, ATTN_Q2P i10, STEM i10) against the uniform
launch of each clip on its own -- bit for bit -- and against the interpreter's reading of the descriptor (tests/mock_exec_mixed.py), at the
smallest shapes that put a clip boundary inside a block."""
import math

import pytest
import torch

from cutie_amd import _lib, ops as O
from cutie_amd.config import default_config
from cutie_amd.model.weights import pack_conv, pack_linear
from oracle import scenarios as S
from oracle.weights import make_state_dict

from mock_exec_mixed import MixedMockExecutor

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope='module')
def gpu_net():
    from cutie_amd.model.cutie import CUTIE
    _lib.set_executor_for_testing(None)
    net = CUTIE(default_config()).cuda().eval()
    net.load_weights(make_state_dict(seed=0))
    return net


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(g, shape, dtype=BF16, dev='cpu', scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(dev)


def bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else t


def against_interpreter(build, seed=0, rtol=None):
    """build(dev, g) -> (OpList, {name: output}): the HIP library and the interpreter with the mixed forms on the same operands (the
    tolerances of tests/test_gpu_kernels.py `check`: bf16 outputs 1.6e-2, fp32 2e-3 of the tensor's scale)."""
    res = []
    for dev, ex in (('cuda', _lib.HipExecutor()), ('cpu', MixedMockExecutor())):
        ol, outs = build(dev, _gen(seed))
        ex.run(ol.finalize())
        if dev == 'cuda':
            torch.cuda.synchronize()
        res.append({k: v.detach().cpu().clone() for k, v in outs.items()})
    hip, ref = res
    for k in ref:
        a, b = hip[k], ref[k]
        assert a.shape == b.shape, (k, a.shape, b.shape)
        if not b.is_floating_point():
            assert torch.equal(a, b), (k, int((a != b).sum()))
            continue
        tol = rtol if rtol is not None else (1.6e-2 if b.dtype == BF16 else 2e-3)
        a, b = a.float(), b.float()
        assert torch.isfinite(a).all(), k
        assert float((a - b).abs().max()) <= tol * float(b.abs().max().clamp(min=1e-6)), (k, float((a - b).abs().max()))


# ---- the whole path ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size,counts,T,cfg_kw', [
    ((240, 432), (1, 4, 2, 3), 14, dict(mem_every=3)),
    ((200, 300), (2, 7), 13, dict(mem_every=2, use_long_term=True, long_term=dict(S.LT_SMALL))),
    # 480p is where the tile table has entries, and it puts the 3x3 convs of 2 and 3 objects on halo tiles, those of 1 and 4 objects on stream
    # tiles: the convs of this group are CUT at the class boundaries (plans.Plan.conv) -- the path no smaller size reaches
    ((480, 854), (1, 2, 3, 4), 9, dict(mem_every=3)),
], ids=['240x432-1.4.2.3', '200x300-2.7-longterm', '480x854-1.2.3.4-cut'])
@pytest.mark.parametrize('hinted', [True, False, 'lanes'])
def test_mixed_lockstep_clips_match_sequential(gpu_net, size, counts, T, cfg_kw, hinted, monkeypatch):
    """Every clip of a mixed group gets the probabilities and the bank of its own InferenceCore run, bit for bit, on one plan per stage."""
    from cutie_amd.inference.inference_core import InferenceCore
    from cutie_amd.inference.lockstep import LockstepCores
    from cutie_amd.utils.synth import SyntheticClip
    monkeypatch.setattr(LockstepCores, 'JOINT', hinted != 'lanes')
    C = len(counts)
    clips = [SyntheticClip(size[0], size[1], k, T, seed=60 + c) for c, k in enumerate(counts)]
    frames = [[cl.frame(t).cuda() for t in range(T)] for cl in clips]
    sizes = lambda mm: {k: (b.n_long, b.n_perm, b.n_work) for k, b in mm.buckets.items()}
    with torch.inference_mode():
        seq = []
        for c, cl in enumerate(clips):
            proc = InferenceCore(gpu_net, cfg=default_config(**cfg_kw))
            outs = [proc.step(frames[c][0], cl.first_mask().cuda(), objects=cl.objects)]
            for t in range(1, T):
                outs.append(proc.step(frames[c][t], end=(t == T - 1)))
            seq.append((torch.stack(outs).cpu(), sizes(proc.memory)))
        ls = LockstepCores(gpu_net, default_config(**cfg_kw), C, mixed_objects=True)
        outs = [ls.step([f[0] for f in frames], [cl.first_mask().cuda() for cl in clips], [cl.objects for cl in clips])]
        for t in range(1, T):
            hint = dict(next_images=[f[t + 1:t + 12] for f in frames]) if hinted and t + 1 < T else {}
            outs.append(ls.step([f[t] for f in frames], end=(t == T - 1), **hint))
        torch.cuda.synchronize()
    assert ls.batched_steps == T - 2
    assert ls.joint_passes == 0                                        # (a mixed group: every clip's own read-out lane)
    if size == (480, 854):                                             # the case is about the cut convs: they must be there
        mixed_plans = [P for P in gpu_net.engine()._plans.values() if getattr(P, 'mixed', None) == counts]
        cut = [sorted({int(r[2][0]) for r in P.ol.recs if r[0] == O.CONV and r[2][11] == 3 and r[2][0] > 1}) for P in mixed_plans]
        assert mixed_plans and any(len(b) > 1 for b in cut), cut        # (3x3 convs over runs of clips, not over the whole group)
    for c in range(C):
        got = torch.stack([o[c] for o in outs]).cpu()
        assert got.shape[1] == counts[c] + 1 and torch.isfinite(got).all()
        assert sizes(ls.cores[c].memory) == seq[c][1], (c, sizes(ls.cores[c].memory), seq[c][1])
        assert torch.equal(got, seq[c][0]), (c, [float((got[t] - seq[c][0][t]).abs().max()) for t in range(T)])


# ---- the mixed forms, op by op ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('md', [True, False])
def test_up4_softmax_mixed(md):
    """UP4_SOFTMAX i5, counts (1, 7, 2) at h4 x w4 = 12 x 20: clip c's K_c + 1 planes (and its MASK_DOWN results) behind those of the clips
    in front = the one-clip launch of every clip."""
    counts, h, w = (1, 7, 2), 12, 20
    st, G = O.clip_starts(counts), len(counts)
    KT, H, W = st[-1], 4 * h, 4 * w
    hw16 = (H // 16) * (W // 16)

    def build(dev, g, per_clip=False):
        lg = (torch.randn((KT, h, w), generator=g) * 3).to(dev)
        prob = torch.zeros((KT + G, H, W), device=dev)
        pair, m16 = torch.zeros((KT, hw16, 64), dtype=BF16, device=dev), torch.zeros((KT, hw16), device=dev)
        ol = O.OpList()
        if per_clip:
            for c, k in enumerate(counts):
                ol.up4_softmax(lg[st[c]:], prob[st[c] + c:], None, P=k + 1, h=h, w=w, from_logits=True,
                               mask_down=(m16[st[c]:], pair[st[c]:], 64) if md else None)
        else:
            ol.up4_softmax(lg, prob, None, P=0, h=h, w=w, from_logits=True, clips=counts, mask_down=(m16, pair, 64) if md else None)
        return ol, {'prob': prob, 'm16': m16, 'pair': pair}
    outs = []
    for per_clip in (False, True):
        ol, o = build('cuda', _gen(6), per_clip)
        ol.run()
        torch.cuda.synchronize()
        outs.append(o)
    for k in outs[0]:
        assert torch.equal(bits(outs[0][k]), bits(outs[1][k])), k
    assert float(outs[0]['prob'].sum()) > 0 and (not md or float(outs[0]['m16'].sum()) > 0)
    against_interpreter(build, seed=6, rtol=2e-3)


def test_upsample2x_add_and_residual_expansion_mixed():
    """UPSAMPLE2X_ADD i6 and the COPY2D i4 expansion + CONV residual that stands for the per-clip broadcast, counts (3, 1, 2) at 6 x 10 pixels
    (one 128-row tile of the conv spans the three clips; a 256-thread block of the others too): = the uniform launch of every clip."""
    counts, h, w, C, Cout, frames = (3, 1, 2), 6, 10, 64, 72, 2
    st, G = O.clip_starts(counts), len(counts)
    KT = st[-1]

    def build(dev, g, per_clip=False):
        x = rnd(g, (KT, h // 2, w // 2, C), dev=dev)
        skip = rnd(g, (G, frames, h, w, C), dev=dev)                  # clip c's map = skip[c, 0]: the maps lie `frames` maps apart
        y = torch.zeros((KT, h, w, C), dtype=BF16, device=dev)
        wt = torch.randn(Cout, C, 1, 1, generator=g) / math.sqrt(C)
        pc = pack_conv(wt, torch.randn(Cout, generator=g) * 0.1, dev)
        res = rnd(g, (G, frames, h, w, Cout), dev=dev)
        rexp = torch.zeros((KT, h, w, Cout), dtype=BF16, device=dev)
        z = torch.zeros((KT, h, w, Cout), dtype=BF16, device=dev)
        ol = O.OpList()
        ol.keep.append(pc.weight)
        kw = dict(H=h, W=w, C1=C, ldx1=C, OH=h, OW=w, ldy=Cout, ldr=Cout, act=O.ACT_RELU, tile=103)
        if per_clip:
            for c, k in enumerate(counts):
                ol.upsample2x_add(x[st[c]:], skip[c, 0], y[st[c]:], B=k, h=h // 2, w=w // 2, C=C)
                ol.conv(y[st[c]:], pc, z[st[c]:], B=k, res=res[c, 0], res_bcast=True, **kw)
        else:
            ol.upsample2x_add(x, skip, y, B=KT, h=h // 2, w=w // 2, C=C, skip_group=(counts, frames * h * w))
            ol.copy2d(res, rexp, rows=KT, rowbytes=h * w * Cout * 2, src_stride=frames * h * w * Cout * 2, dst_stride=h * w * Cout * 2, clips=counts)
            ol.conv(y, pc, z, B=KT, res=rexp, **kw)
        return ol, {'y': y, 'z': z}
    outs = []
    for per_clip in (False, True):
        ol, o = build('cuda', _gen(4), per_clip)
        ol.run()
        torch.cuda.synchronize()
        outs.append(o)
    for k in outs[0]:
        assert torch.equal(bits(outs[0][k]), bits(outs[1][k])), k
    assert float(outs[0]['z'].float().abs().sum()) > 0
    against_interpreter(build, seed=4)


@pytest.mark.parametrize('qpre', [0, 1])
def test_q2p_chain_mixed(qpre):
    """ATTN_Q2P i10 (chain form), counts (1, 5) at HW = 60: the foreground masks are decided among the objects of the object's own clip -- the
    launch adds to the accumulator exactly what the launch of every clip on its own adds (K = 1: the KT = 4 kernel, K = 5: KT = 8)."""
    counts, Q, HW, C, heads = (1, 5), 16, 60, 256, 8
    st = O.clip_starts(counts)
    K = st[-1]
    M = K * Q

    def build(dev, g, per_clip=False):
        lg = (torch.randn((K, HW), generator=g) * 2).to(dev)
        x, emb = torch.randn((M, C), generator=g).to(dev), (torch.randn((M, C), generator=g) * 0.5).to(dev)
        gam, bet = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.1).to(dev)
        Wq = pack_linear(torch.randn((C, C), generator=g) / 16, torch.randn(C, generator=g) * 0.1, dev)
        Wo = pack_linear(torch.randn((C, C), generator=g) / 16, torch.randn(C, generator=g) * 0.1, dev)
        kvq = rnd(g, (K, HW, 3 * C), dev=dev)
        qs = (torch.randn((M, C), generator=g) * 0.2).to(dev)
        acc = torch.zeros((M, C), dtype=torch.int64, device=dev)
        xn = torch.zeros((M, C), dtype=F32, device=dev)
        ol = O.OpList()
        ol.keep += [Wq.weight, Wo.weight, Wq.bias, Wo.bias]
        common = dict(Q=Q, HW=HW, C=C, heads=heads, ldkv=3 * C, voff=C)

        def launch(k0, k1, clip_objects):
            if qpre:
                ol.attn_q2p(None, kvq[k0:], None, None, None, K=k1 - k0, logits=lg[k0:], q_pre=qs[k0 * Q:], out_proj=(Wo, acc[k0 * Q:]), clip_objects=clip_objects, **common)
            else:
                ol.attn_q2p(None, kvq[k0:], None, None, None, K=k1 - k0, logits=lg[k0:], proj=dict(x=x[k0 * Q:], W=Wq, emb=emb[k0 * Q:], ln=(gam, bet), ln_out=xn[k0 * Q:]),
                            out_proj=(Wo, acc[k0 * Q:]), clip_objects=clip_objects, **common)
        if per_clip:
            for c in range(len(counts)):
                launch(st[c], st[c + 1], None)
        else:
            launch(0, K, counts)
        return ol, {'acc': acc, 'xn': xn}
    outs = []
    for per_clip in (False, True, 'one'):
        ol, o = build('cuda', _gen(11), per_clip is True)
        if per_clip == 'one':                                          # all six objects as ONE clip: other masks
            ol.recs[0][2][10] = 0
        ol.run()
        torch.cuda.synchronize()
        outs.append(o)
    assert torch.equal(outs[0]['acc'], outs[1]['acc']) and torch.equal(outs[0]['xn'], outs[1]['xn'])
    assert not torch.equal(outs[0]['acc'], outs[2]['acc'])
    # the interpreter: the fixed-point accumulator in units of 2^-32, as a float
    def build_f(dev, g):
        ol, o = build(dev, g)
        return ol, {'xn': o['xn'], 'acc_holder': o['acc']}
    res = []
    for dev, ex in (('cuda', _lib.HipExecutor()), ('cpu', MixedMockExecutor())):
        ol, o = build_f(dev, _gen(11))
        ex.run(ol.finalize())
        if dev == 'cuda':
            torch.cuda.synchronize()
        res.append((o['acc_holder'].cpu().double() / O.OpList.QACC_SCALE).float())
    assert float((res[0] - res[1]).abs().max()) <= 2e-3 * float(res[1].abs().max()), float((res[0] - res[1]).abs().max())


def test_stem_mixed():
    """STEM i10, counts (2, 1, 3) at 32 x 48: the clips as the frames of one launch, each with its own object count -- clip c's masks are the
    planes (start_c + c + 1) .. of the group's probability tensor, its output the objects start_c ..: = one launch per clip."""
    counts, h0, w0, H, W, pl, pt = (2, 1, 3), 30, 43, 32, 48, 1, 1
    st, G = O.clip_starts(counts), len(counts)
    KT = st[-1]
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]

    def build(dev, g, per_clip=False):
        imgs = [torch.rand((3, h0, w0), generator=g).to(dev) for _ in range(G)]
        masks = torch.rand((KT + G, H, W), generator=g)
        masks = (masks * (torch.rand((KT + G, H, W), generator=g) > 0.5)).to(dev)
        wt = torch.randn((64, 8, 7, 7), generator=g) / math.sqrt(147)
        wt[:, 5:] = 0
        pc = pack_conv(wt, torch.randn(64, generator=g) * 0.1, dev)
        y = torch.zeros((KT, H // 4, W // 4, 64), dtype=BF16, device=dev)
        kw = dict(h0=h0, w0=w0, H=H, W=W, pad_left=pl, pad_top=pt, mean=mean, std=std, relu=True)
        ol = O.OpList()
        ol.keep += [pc.weight, pc.bias]
        if per_clip:
            for c, k in enumerate(counts):
                ol.stem(imgs[c], masks[st[c] + c + 1:], pc, y[st[c]:], K=k, **kw)
        else:
            ol.stem(imgs[0], masks[1:], pc, y, K=0, more_images=imgs[1:], counts=counts, **kw)
        return ol, {'y': y}
    outs = []
    for per_clip in (False, True):
        ol, o = build('cuda', _gen(17), per_clip)
        ol.run()
        torch.cuda.synchronize()
        outs.append(o)
    assert torch.equal(bits(outs[0]['y']), bits(outs[1]['y'])) and float(outs[0]['y'].float().abs().sum()) > 0
    against_interpreter(build, seed=17)


def test_the_library_announces_the_mixed_forms():
    assert _lib.has_mixed_lockstep()
