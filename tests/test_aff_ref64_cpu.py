"""tests/aff_ref64.py on the host: the float64 chain agrees with the reference algorithm (oracle.net.get_similarity / topk_softmax) run in
float64; the interpreter's fp32 results (tests/mock_exec.py) lie inside every stage's bound and pass every exact check; the share of
ambiguous queries stays under the cap for every seed the GPU file uses; and the checks bite: each fault a read-out kernel can plausibly make,
applied to the interpreter's outputs or to an fp32 restatement of the stage, fails at least one of them."""
import pytest
import torch

import aff_ref64 as A
from cutie_amd import ops as O
from mock_exec import MockExecutor
from oracle.net import get_similarity, topk_softmax

BF16 = torch.bfloat16


def _mock(ol):
    MockExecutor().run(ol.finalize())


# ---- the float64 chain against the reference algorithm ---------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', ['randn0.8', 'video3', 'cluster'])
def test_pipeline_ref_is_the_reference_algorithm_in_float64(regime):
    HW, ranges, top_k = 65, [(3, 200), (300, 117)], 30
    nslots = 420
    mkey, mshr, qkey, qsel = A.make_keys(11, regime, HW, ranges, nslots)
    g = torch.Generator().manual_seed(1)
    vals = [torch.randn((nslots, 16), generator=g).to(BF16) for _ in range(2)]
    ref = A.pipeline_ref(mkey, mshr, qkey[0], qsel[0], ranges, vals, top_k, nslots)
    sl = A.slots_of(ranges)
    sim = get_similarity(mkey[sl].t().double(), mshr[sl].double(), qkey[0].t().double(), qsel[0].t().double())
    scale = max(1.0, float(ref['mag'].max()))
    assert float((sim.t() - ref['S']).abs().max()) <= 1e-12 * scale
    aff, usage = topk_softmax(sim, top_k)
    assert float((aff.t() - ref['W']).abs().max()) <= 1e-9        # (weights: the two expansions' logits differ by 1e-12 scale, relatively in e^x)
    assert float((usage - ref['usage'][sl]).abs().max()) <= 1e-9 * HW
    ok = ~ref['ambiguous']
    for o, v in enumerate(vals):
        dense = (v[sl].double().t() @ aff).t()
        assert float((dense - ref['y'][o])[ok].abs().max()) <= 1e-8


# ---- the interpreter passes every stage check --------------------------------------------------------------------------------------------
def _chain(regime, seed, HW=A.CHAIN_HW, ranges=A.CHAIN_RANGES, K=2, top_k=30, form='nq2', frames=1, usage_fx=True):
    c = A.AffCase('cpu', HW=HW, ranges=ranges, regime=regime, seed=seed, K=K, top_k=top_k, frames=frames)
    p = c.passes('a')
    ol = O.OpList()
    c.prep(ol)
    c.score0(ol, p, form)
    c.select(ol, p)
    c.score1(ol, p, form)
    y, use, ovf = c.readout(ol, p, 'a', usage_fx=usage_fx)
    _mock(ol)
    return c, p, y, use, ovf


@pytest.mark.parametrize('regime,seed', A.CHAIN_CASES)
def test_the_interpreter_lies_inside_every_stage_bound(regime, seed):
    fx = regime != 'video8'
    c, p, y, use, ovf = _chain(regime, seed, usage_fx=fx)
    sl = A.slots_of(c.ranges)
    r = A.key_prep_ref(c.mkey[sl], c.mshr[sl], False)
    A.check_key_prep(c.Ahi[sl], c.Alo[sl], c.scale[sl], r, 'memory side')
    r = A.key_prep_ref(c.qkey[0], c.qsel[0], True)
    A.check_key_prep(c.Bhi, c.Blo, c.cq, r, 'query side')
    sref = c.score_ref()
    A.verify_score0(c, p, sref=sref, pad_written=False)
    A.verify_select(c, p)
    A.verify_score1(c, p, sref=sref)
    A.verify_readout(c, p, y, use, ovf)
    assert c.b.guards_intact()
    _verify_chain(c, y, use)


def _verify_chain(c, y, use, f=0):
    ref = A.pipeline_ref(c.mkey, c.mshr, c.qkey[f], c.qsel[f], c.ranges, c.values, c.top_k, c.nslots)
    assert float(ref['ambiguous'].float().mean()) <= A.AMBIG_CAP
    ok = ~ref['ambiguous']
    got = y[f].detach().cpu().double()
    r = A.check_bound(got[:, ok].reshape(-1, c.CV), ref['y'][:, ok].reshape(-1, c.CV), ref['ybound'][:, ok].reshape(-1, c.CV), what='chain y')
    A.check_bound(A.usage_float(use[f]).view(-1, 1), ref['usage'].view(-1, 1), ref['ubound'].view(-1, 1) + 1e-30, what='chain usage')
    return r


def test_stacked_frames_on_the_interpreter():
    c, p, y, use, ovf = _chain('video3', 5, HW=50, ranges=[(2, 300)], frames=3, top_k=5)
    for f in range(3):
        A.verify_score0(c, p, f, pad_written=False)
        A.verify_select(c, p, f)
        A.verify_score1(c, p, f)
        A.verify_readout(c, p, y, use, ovf, f)
    assert c.b.guards_intact()


# ---- the cap: ambiguous queries per seed and regime of the GPU file ------------------------------------------------------------------
@pytest.mark.parametrize('regime,seed', A.CHAIN_CASES)
def test_share_of_ambiguous_queries_stays_under_the_cap(regime, seed):
    for frames in (1, 3):
        mkey, mshr, qkey, qsel = A.make_keys(seed, regime, A.CHAIN_HW, A.CHAIN_RANGES, A.CHAIN_NSLOTS, frames)
        vals = [torch.zeros((A.CHAIN_NSLOTS, 8), dtype=BF16)]
        for f in range(frames):
            ref = A.pipeline_ref(mkey, mshr, qkey[f], qsel[f], A.CHAIN_RANGES, vals, 30, A.CHAIN_NSLOTS)
            share = float(ref['ambiguous'].float().mean())
            print(f'aff_ref64 ambiguous {regime} seed={seed} frames={frames} f={f}: {int(ref["ambiguous"].sum())} of {A.CHAIN_HW} ({share:.3f})')
            assert share <= A.AMBIG_CAP


def test_hand_built_lists_leave_out_no_query():
    """The read-out's reference works from the list as given with the exact selection rule: no query is ever left out of it."""
    cv, ci, cnt, groups = A.hand_lists(top_k=30, cap=1024, nslots=2000)
    ref = A.readout_ref(cv, ci, cnt, [torch.ones((2000, 8), dtype=BF16)], 30, 1024, 2000)
    assert bool(torch.isfinite(ref['ybound']).all()) and bool(torch.isfinite(ref['y']).all())
    w = ref['y'][0, :, 0]
    assert bool(((w - 1).abs() <= 1e-12)[cnt > 0].all()) and bool((w[cnt == 0] == 0).all())          # the weights of every list sum to one
    for grp in groups:
        assert all(torch.equal(ref['y'][0, grp[0]], ref['y'][0, r]) or float((ref['y'][0, grp[0]] - ref['y'][0, r]).abs().max()) < 1e-12 for r in grp)


# ---- the bounds bite ---------------------------------------------------------------------------------------------------------------------
def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_fault_lo_hi_term_dropped_and_c_over_63_channels():
    c = A.AffCase('cpu', HW=33, ranges=[(0, 100)], regime='video3', seed=2)
    ol = O.OpList()
    c.prep(ol)
    _mock(ol)
    sref = c.score_ref()
    gm, gb = A.tile_max_ref(sref['S'], sref['bound'], c.ranges)
    sl = A.slots_of(c.ranges)
    ah, al, bh, bl = c.Ahi[sl].float(), c.Alo[sl].float(), c.Bhi[:33].float(), c.Blo[:33].float()
    cq, sc = c.cq[:33], c.scale[sl]
    good = (bh @ ah.t() + bl @ ah.t() + bh @ al.t() - cq[:, None]) * sc[None]
    A.check_bound(good, sref['S'], sref['bound'], what='fp32 three-term score')
    dropped = (bh @ ah.t() + bl @ ah.t() - cq[:, None]) * sc[None]
    assert _fails(lambda: A.check_bound(dropped, sref['S'], sref['bound']))
    c63 = (c.qsel[0] * c.qkey[0] * c.qkey[0])[:, :63].sum(1)
    r = A.key_prep_ref(c.qkey[0], c.qsel[0], True)
    assert _fails(lambda: A.check_key_prep(c.Bhi, c.Blo, c63, r))
    short = (bh @ ah.t() + bl @ ah.t() + bh @ al.t() - c63[:, None]) * sc[None]
    assert _fails(lambda: A.check_bound(short, sref['S'], sref['bound']))


def test_fault_threshold_tie_padding_row_and_ragged_tile():
    c, p, y, use, ovf = _chain('randn0.8', 9, HW=33, ranges=[(4, 37), (64, 200)], top_k=5)
    sref = c.score_ref()
    A.verify_score1(c, p, sref=sref)
    keep = c.b.snapshot()

    def restore():
        for n, v in keep.items():
            c.b[n].copy_(v)
    # `>` in place of `>=` at the threshold: the token that made the top_k-th tile maximum is lost
    cnt = c.counts(p)
    tau = c.frame_rows(p['tau'])
    for j in range(c.HW):
        n = int(cnt[j])
        v, i = p['cval'][j, :n].clone(), p['cidx'][j, :n].clone()
        m = v > tau[j]
        k = int(m.sum())
        p['cval'][j, :k], p['cidx'][j, :k] = v[m], i[m]
        p['cval'][j, k:n], p['cidx'][j, k:n] = A.SENT_F, A.SENT_I
        cnt[j] = k
    assert _fails(lambda: A.verify_score1(c, p, sref=sref))
    restore()
    # a query row of the padding written
    p['count'].view(-1, 32)[c.HW, 0] = 1
    assert _fails(lambda: A.verify_score1(c, p, sref=sref))
    restore()
    p['tau'][c.HW] = 0.0
    assert _fails(lambda: A.verify_select(c, p))
    restore()
    # the token behind a ragged tile's last valid one included in the maximum: range 0 ends at slot 40, the maximum takes slot 41 too, which no
    # range holds -- such slots score 0 (make_keys), above every real score
    extra = A.score_ref(c.Ahi, c.Alo, c.scale, c.Bhi, c.Blo, c.cq, [(4, 38)], c.HW)['S']
    assert bool((extra[:, 37] == 0).all())
    gm, gb = A.tile_max_ref(sref['S'], sref['bound'], c.ranges)
    bad = gm.clone()
    bad[:, 2] = torch.maximum(gm[:, 2], extra[:, 37])
    assert _fails(lambda: A.check_bound(bad, gm, gb))
    # and the selection: the k-th largest, not the (k+1)-th or (k-1)-th
    g = c.frame_rows(p['gmax'])[:, :c.G]
    assert bool((A.select_ref(g, 5) != A.select_ref(g, 6)).any()) and bool((A.select_ref(g, 5) == g.topk(5, dim=1).values[:, -1]).all())


def _readout_fp32(cv, ci, cnt, V, top_k, fault=None):
    """An fp32 restatement of AFF_READOUT for one query (prune included), with the faults of the issue on demand.  Returns (y, {token: weight})."""
    n = int(cnt)
    v, i = cv[:n].clone(), ci[:n].clone().long()
    nsel = min(n, top_k)
    if n > A.RO_PRUNE:
        kth = torch.sort(v, descending=True).values[nsel - 1]
        keep = v >= kth
        if fault == 'rank_before_prune':                       # the ranking runs over the first `kept` entries of the list as it was
            v, i = v[:int(keep.sum())], i[:int(keep.sum())]
        else:
            v, i = v[keep], i[keep]
    lower = (i[None] > i[:, None]) if fault == 'tie_reversed' else (i[None] < i[:, None])
    rank = (v[None] > v[:, None]).sum(1) + ((v[None] == v[:, None]) & lower).sum(1)
    sv, si = torch.full((nsel,), A.NEG_INF), torch.full((nsel,), int(ci[0]), dtype=torch.int64)
    m = rank < nsel
    sv[rank[m]], si[rank[m]] = v[m], i[m]
    e = torch.where(sv > A.NEG_INF, torch.exp(sv - sv[0]), torch.zeros(()))
    w = e / (e.sum() + (torch.exp(v - sv[0]).sum() - e.sum() if fault == 'norm_over_cnt' else 0.0))
    return (w[:, None] * V[si].float()).sum(0).to(BF16), si, w


@pytest.mark.parametrize('fault', [None, 'tie_reversed', 'rank_before_prune', 'norm_over_cnt', 'trunc32'])
def test_faults_of_the_read_out(fault):
    top_k, cap, nslots = 30, 1024, 2000
    g = torch.Generator().manual_seed(4)
    V = torch.randn((nslots, 32), generator=g).to(BF16)
    caught = False
    cv, ci, cnt, _ = A.hand_lists(top_k=top_k, cap=cap, nslots=nslots)
    for name in ('hand lists',):
        HW = cnt.numel()
        ref = A.readout_ref(cv, ci, cnt, [V], top_k, cap, nslots)
        y = torch.zeros((HW, 32), dtype=BF16)
        use = torch.zeros(nslots, dtype=torch.int64)
        for j in range(HW):
            if int(cnt[j]) == 0:
                continue
            y[j], si, w = _readout_fp32(cv[j], ci[j], cnt[j], V, top_k, fault)
            fx = (w * 2.0 ** 40).to(torch.int64)
            if fault == 'trunc32':
                fx = (w * 2.0 ** 32).to(torch.int64) << 8
            use.index_add_(0, si, fx)
        bad = _fails(lambda: A.check_bound(y, ref['y'][0], ref['ybound'][0], what=name)) or \
            _fails(lambda: A.check_bound(A.usage_float(use).view(-1, 1), ref['usage'].view(-1, 1), ref['ubound_fx'].view(-1, 1) + A.FX * 1e-6, what=name))
        assert fault is not None or not bad, name
        caught |= bad
    assert caught == (fault is not None)
