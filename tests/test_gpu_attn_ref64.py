"""The object transformer's query side (csrc/attention.hip, csrc/qchain.hip) on the MI355X against the float64 references of
tests/attn_ref64.py, element by element: one launch per case, built by tests/attn_cases.py between NaN / sentinel guard rows; every output
within its derived bound (ref64.check_bound), the sentinels intact, a second run of the same launch bit-identical (accumulators included),
mask bytes and counts exact.  The shapes are the smallest at which each path can go wrong: HW around the 32-pixel chunk, the 8-wave
round, the prefetch depth (1024), the 2048-pixel early / late split of the mask logits and the 256-pixel block / 64-pixel wave of
ATTN_P2Q; K on both sides of the 4 / 8 object variants; one case at the largest HW the chain form accepts (the only one above 64 KB of
LDS per workgroup) and the refusal one pixel above it.  Each test prints its worst |err| / bound (DESIGN.md keeps the table)."""
import os
import re

import pytest
import torch

import attn_cases as AC
import attn_ref64 as A
import ref64 as R
from cutie_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda'


ONE_WRITER = ('ln_out', 'xn_out', 'x_out')


def run_case(c, names, tag, exact=()):
    ex = _lib.HipExecutor()
    arr = c.ol.finalize()
    ex.run(arr)
    torch.cuda.synchronize()
    first = {n: c.raw(n).clone() for n in c.outs}
    ref = c.ref()
    worst = {}
    for n in names:
        y, b = ref[n]
        worst[n] = R.check_bound(c.got(n), y, b, what=f'{tag}:{n}')
    for n in ONE_WRITER:
        if n in c.outs:
            # ln_out / xn_out / x_out are written by ONE block per object (head 0, slice 0, the last pixel block's head 0).  Every block computes these
            # rows with the same instructions from the same operands, so a second writer would store the same bits: what can be observed is
            # that every element WAS written (the rows start as NaN), lies inside its bound (checked above for every name a case lists), is
            # the same after a second run, and that nothing next to the rows was touched (the sentinels below)
            assert n in names and bool(torch.isfinite(c.raw(n)).all()), (tag, n, 'a row that one block must write was left unwritten')
    for n in exact:
        want = ref['fg'].to(torch.uint8) if n == 'aux_fg' else ref['n_fg'].to(torch.int32)
        assert torch.equal(c.raw(n), want.view_as(c.raw(n))), (tag, n, int((c.raw(n) != want.view_as(c.raw(n))).sum()))
    assert c.guards_intact(), (tag, 'a sentinel next to an output was overwritten')
    c.reset()
    ex.run(arr)
    torch.cuda.synchronize()
    for n, t in first.items():
        a, b = c.raw(n), t
        same = torch.equal(a, b) if not a.is_floating_point() else torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32),
                                                                               b.view(torch.int16 if b.element_size() == 2 else torch.int32))
        assert same, (tag, n, 'a second run of the same launch differs')
    assert c.guards_intact()
    print('attn_ref64 ratio', tag, ' '.join(f'{n}={v:.3g}' for n, v in worst.items()))
    return worst


def _q2p_names(form):
    return (['acc'] if form.startswith('chain') else ['y']) + (['ln_out'] if form in ('proj', 'chain', 'chain_acc') else [])


# ---- ATTN_Q2P, chain form: HW x layout, K / form cycling through the nine instantiations ------------------------------------------------
HWS = [1, 31, 32, 33, 37, 255, 256, 257, 1024, 1025, 2047, 2048, 2049]
KS = [1, 4, 5, 8, 9]
CH_FORMS = ['chain', 'chain_acc', 'chain_qpre']
REGIMES = ['randn', 'large', 'sparse']
Q2P_CHAIN = []
for hi_, HW in enumerate(HWS):
    for li, layout in enumerate(('sep', 'inter')):
        n = 2 * hi_ + li
        # K walks 1, 4, 5, 8, 9 and the form chain, chain_acc, chain_qpre: 15 steps cover every (K, form) pair, hence all nine instantiations
        Q2P_CHAIN.append((HW, KS[n % 5], CH_FORMS[n % 3], layout, REGIMES[(n // 3) % 3]))


def test_the_chain_cases_reach_every_instantiation_layout_and_size():
    kt = lambda K: 4 if K <= 4 else 8 if K <= 8 else 0
    assert {(f, kt(K)) for _, K, f, _, _ in Q2P_CHAIN} == {(f, t) for f in CH_FORMS for t in (0, 4, 8)}
    assert {(HW, lay) for HW, _, _, lay, _ in Q2P_CHAIN} == {(HW, lay) for HW in HWS for lay in ('sep', 'inter')}
    assert {K for _, K, _, _, _ in Q2P_CHAIN} == set(KS) and {r for *_, r in Q2P_CHAIN} == set(REGIMES)
    assert {kt(K) for h, K, _, _, _ in Q2P_CHAIN if h in (2047, 2048, 2049)} == {0, 4, 8}       # the early / late split of the logits, every variant


@pytest.mark.parametrize('HW,K,form,layout,regime', Q2P_CHAIN)
def test_q2p_chain(HW, K, form, layout, regime):
    c = AC.build_q2p(DEV, K=K, HW=HW, form=form, layout=layout, regime=regime, gap=(HW % 2 == 1), seed=HW * 16 + K)
    run_case(c, _q2p_names(form), f'q2p {form} {regime} HW={HW} K={K} {layout}')


@pytest.mark.parametrize('K,Kg,HW,form,layout', [(6, 3, 257, 'chain_acc', 'inter'), (10, 5, 300, 'chain', 'sep'), (10, 5, 2049, 'chain_qpre', 'inter'),
                                                (6, 3, 33, 'chain_qpre', 'sep')])
def test_q2p_chain_clips(K, Kg, HW, form, layout):
    """Clips in lock step: the mask of an object is decided among the Kg objects of its clip; one clip has a saturated plane."""
    c = AC.build_q2p(DEV, K=K, HW=HW, form=form, layout=layout, Kg=Kg, sat={Kg: -20.0}, seed=K + HW)
    run_case(c, _q2p_names(form), f'q2p {form} clips K={K}/{Kg} HW={HW}')


FEW = [(37, 0), (37, 1), (37, 2), (37, 5), (37, 32), (37, 36), (37, 37), (2049, 1), (2049, 2048), (2049, 2049), (2049, 0)]


@pytest.mark.parametrize('form,HW,n', [('chain_qpre', HW, n) for HW, n in FEW if HW == 37 or n in (1, HW - 1)] + [('q_lg', HW, n) for HW, n in FEW if HW == 37] +
                         [('chain', HW, n) for HW, n in FEW if n in (0, HW) or (HW == 37 and n in (1, HW - 1))])
def test_q2p_few_visible_pixels(form, HW, n):
    """n_fg in {0, 1, 2, 5, HW - 5, HW - 1, HW}: a query sees a handful of pixels (no averaging to hide a lost term behind), pixel 0 and pixel
    HW - 1 among them; 0 and HW are the two sides of the unblocking rule.  'chain_qpre' and 'q_lg' are the forms whose bound sees a lost lo term
    here; 'chain' runs the two sides of the unblocking rule and one pixel on either side of them."""
    K = 3 if HW == 37 else 5
    c = AC.build_q2p(DEV, K=K, HW=HW, form=form, regime='few', n_fg={1: n}, layout='inter' if form == 'chain' else 'sep', seed=HW + n)
    assert int(c.info['n_fg'][1]) == n
    run_case(c, _q2p_names(form), f'q2p {form} few HW={HW} n_fg={n}')


@pytest.mark.parametrize('mode', ['nofg', 'allfg'])
@pytest.mark.parametrize('form', ['chain_acc', 'q_lg', 'proj'])
def test_q2p_saturated_planes(form, mode):
    """Planes at exactly -20 / +20 (the degenerate masks of test_gpu_kernels.py) and -30 / +30: ties at the clamp are foreground."""
    sat = {0: -20.0} if mode == 'nofg' else {0: -20.0, 2: -30.0, 1: 20.0, 3: -20.0}
    c = AC.build_q2p(DEV, K=4, HW=1620, form=form, sat=sat, seed=7, aux=(form != 'chain_acc'))
    n = c.info['n_fg']
    assert int(n[0]) == 0 and (mode == 'nofg' or int(n[1]) == 1620)
    run_case(c, _q2p_names(form), f'q2p {form} {mode}', exact=('aux_fg', 'aux_nfg') if form != 'chain_acc' else ())


# ---- ATTN_Q2P, the forms of attention.hip, with AUX_MASK on the same logits ---------------------------------------------------------------
@pytest.mark.parametrize('HW,K,form,regime', [(1, 1, 'q_fg', 'randn'), (37, 4, 'q_lg', 'large'), (257, 5, 'proj', 'sparse'), (1025, 9, 'q_fg', 'large'),
                                              (2049, 8, 'q_lg', 'randn'), (33, 9, 'proj', 'large'), (1024, 1, 'proj', 'randn'), (2048, 4, 'q_lg', 'sparse')])
def test_q2p_plain_forms_and_aux_mask(HW, K, form, regime):
    c = AC.build_q2p(DEV, K=K, HW=HW, form=form, regime=regime, gap=(HW % 2 == 1), seed=HW + K, aux=True)
    run_case(c, _q2p_names(form), f'q2p {form} {regime} HW={HW} K={K}', exact=('aux_fg', 'aux_nfg'))


# ---- the largest HW of the chain form: more than 64 KB of LDS per workgroup -------------------------------------------------------------
def _chain_hw_limit():
    """From launch_qchain's own check: dyn = HWp + NWV * 32 * Q2C_VLD * 2 <= 96 * 1024, HWp = HW rounded up to 16."""
    src = open(os.path.join(os.path.dirname(_lib.__file__), 'csrc', 'qchain.hip')).read()
    vld = int(re.search(r'#define\s+Q2C_VLD\s+(\d+)', src).group(1))
    nwv = int(re.search(r'constexpr int NWV = (\d+);', src).group(1))
    m = re.search(r'dyn = \(size_t\)HWp \+ NWV \* 32 \* Q2C_VLD \* 2;\s*if \(dyn > (\d+) \* 1024\)', src)
    assert m, 'the LDS check of the chain form of ATTN_Q2P has changed: derive the limit anew'
    return (int(m.group(1)) * 1024 - nwv * 32 * vld * 2) // 16 * 16


def test_q2p_chain_at_the_largest_hw():
    HW = _chain_hw_limit()
    assert HW + 8 * 32 * 40 * 2 > 64 * 1024
    c = AC.build_q2p(DEV, K=1, HW=HW, form='chain_acc', layout='inter', seed=3)
    run_case(c, ['acc', 'ln_out'], f'q2p chain_acc HW={HW} (LDS > 64 KB)')


def test_q2p_chain_one_pixel_above_the_limit_is_refused():
    HW = _chain_hw_limit() + 1
    c = AC.build_q2p(DEV, K=1, HW=HW, form='chain_acc', layout='inter', seed=3)        # buffers sized for this HW
    before = {n: c.raw(n).clone() for n in c.outs}
    with pytest.raises(RuntimeError, match='does not fit the LDS'):
        _lib.HipExecutor().run(c.ol.finalize())
    torch.cuda.synchronize()
    assert torch.equal(c.raw('acc'), before['acc']) and bool(torch.isnan(c.raw('ln_out')).all()) and c.guards_intact()      # nothing launched


# ---- ATTN_SELF, ATTN_P2Q, QFFN, QUERY_INIT --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('K,form', [(5, 'plain'), (3, 'proj'), (1, 'chain'), (5, 'chain')])
def test_attn_self(K, form, regime):
    names = ['acc', 'ln_out'] if form == 'chain' else ['y'] + (['ln_out'] if form == 'proj' else [])
    run_case(AC.build_self(DEV, K=K, form=form, regime=regime, seed=K), names, f'self {form} {regime} K={K}')


P2Q = [(1, 1, 'chain', 1, 'randn'), (63, 2, 'chain', 0, 'large'), (64, 1, 'chain', 1, 'sparse'), (65, 3, 'chain', 0, 'randn'), (255, 1, 'chain', 1, 'large'),
       (256, 2, 'chain', 0, 'randn'), (257, 1, 'chain', 1, 'randn'), (1025, 2, 'chain', 1, 'sparse'), (37, 3, 'plain', 0, 'randn'), (257, 1, 'plain', 0, 'large'),
       (1, 1, 'proj', 0, 'randn'), (256, 2, 'proj', 0, 'sparse'), (321, 1, 'proj', 0, 'large')]


@pytest.mark.parametrize('HW,K,form,nq,regime', P2Q)
def test_attn_p2q(HW, K, form, nq, regime):
    c = AC.build_p2q(DEV, K=K, HW=HW, form=form, next_q=bool(nq), regime=regime, gap=(HW % 2 == 1), seed=HW + K)
    run_case(c, ['y'] + (['q_out', 'xn_out'] if nq else []), f'p2q {form} {regime} HW={HW} K={K} next_q={nq}')


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('K,hs', [(1, 64), (3, 128)])
def test_qffn(K, hs, regime):
    run_case(AC.build_qffn(DEV, K=K, hid_slice=hs, regime=regime, seed=K + hs), ['acc', 'x_out'], f'qffn {hs} {regime} K={K}')


@pytest.mark.parametrize('K,regime', [(1, 'randn'), (3, 'sparse'), (5, 'large'), (5, 'sparse')])
def test_query_init_with_its_linears(K, regime):
    run_case(AC.build_qinit(DEV, K=K, regime=regime, seed=K), ['query', 'query_emb'], f'query_init2 {regime} K={K}')
