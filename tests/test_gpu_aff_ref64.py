"""The pixel-memory read-out (csrc/affinity.hip) on the MI355X against the float64 references of tests/aff_ref64.py, stage by stage and
element by element: one small launch sequence per case, every output between sentinel elements that must survive, every value within its
derived bound, every exact property (selection, ties, bit-identity between the kernel forms and between the two passes) asserted as such,
and a second run of the same launches bit-identical wherever the kernel is deterministic (everything except the ORDER of the candidate
entries and the f32-atomics usage).  Each test prints its worst |err| / bound; DESIGN.md keeps the table.

What the candidate lists are held to (aff_ref64.check_candidates): count <= cap; no token twice; every value >= tau and within the bound of
S_op; everything clearly above tau present, nothing clearly below; count >= min(top_k, N) whenever G >= top_k; for every tile whose pass-0
maximum reaches tau the best listed value of that tile IS that maximum, bit for bit; entries past count and the lists of padding rows keep
their sentinels."""
import pytest
import torch

import aff_ref64 as A
from cutie_amd import _lib
from cutie_amd import ops as O
from oracle.net import get_similarity

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, BF16, I32, I64 = torch.float32, torch.bfloat16, torch.int32, torch.int64
FORMS = list(A.FORMS)


def launch(ol):
    ex, arr = _lib.HipExecutor(), ol.finalize()
    ex.run(arr)
    torch.cuda.synchronize()
    return ex, arr


def rerun_is_identical(b, ex, arr, skip=()):
    """A second run of the same launches leaves the same bits in every output whose name does not start with one of `skip`."""
    first = b.snapshot()
    b.reset()
    ex.run(arr)
    torch.cuda.synchronize()
    for n, t in first.items():
        if not (skip and n.startswith(tuple(skip))):
            assert torch.equal(A.bits(b[n]), A.bits(t)), (n, 'a second run of the same launch differs')
    assert b.guards_intact()


# ---- KEY_PREP ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('query', [False, True])
@pytest.mark.parametrize('n', [1, 15, 16, 17, 257])
def test_key_prep(n, query):
    worst = {}
    for ri, regime in enumerate(A.REGIMES[:5]):
        mkey, mshr, qkey, qsel = A.make_keys(n + ri, regime, n, [(0, n)], n)
        key, aux = (qkey[0], qsel[0]) if query else (mkey, mshr)
        key = key.clone()
        key[0, 0], key[0, 1], key[n - 1, 63] = 0.0, 2.0 ** 60, 0.0                   # zeros, and one value whose square is still finite in fp32
        if query:
            aux = aux.clone()
            aux[0, 2] = 0.0
        b = A.Bufs(DEV)
        hi, lo, side = b.output('hi', (n, 128), BF16), b.output('lo', (n, 128), BF16), b.output('side', (n,), F32)
        ol = O.OpList()
        ol.key_prep(b.operand(key), b.operand(aux), hi, lo, side, n=n, query=query)
        ex, arr = launch(ol)
        ref = A.key_prep_ref(key, aux, query)
        assert bool(torch.isfinite(ref['v']).all()) and bool(torch.isfinite(ref['vbound']).all())
        worst[regime] = A.check_key_prep(hi, lo, side, ref, f'key_prep {regime} n={n} query={query}')
        if not query:
            assert torch.equal(side.cpu(), aux * 0.125)                                # scale is exact
        assert b.guards_intact()
        rerun_is_identical(b, ex, arr)
    print('aff_ref64 ratio key_prep', 'query' if query else 'memory', f'n={n}', ' '.join(f'{k}={v:.3g}' for k, v in worst.items()))


# ---- AFF_SCORE, both passes, every form reachable without the bank table ---------------------------------------------------------------
# (HW, ranges, regime, top_k): HW straddles the 16-query set, the 64 / 128 / 256 rows of a block (1, 2, 4 sets per wave) and the HWp padding; the
# ranges start off the 16-token grid and end in ragged tiles; G walks around the 4-tile LDS group, top_k and the 64-column row of gmax; 19 tiles
# are 5 groups (block rows of 2 and 3 groups); the last case is the size class of a long clip.
SCORE_CASES = [
    (1, [(3, 1)], 'randn0.8', 5), (63, [(3, 37)], 'video3', 5), (64, [(5, 64)], 'video8', 5), (65, [(5, 65)], 'sparse_sel', 5),
    (127, [(1, 128)], 'randn0.8', 5), (128, [(1, 129)], 'video3', 5), (129, [(3, 15), (32, 17), (100, 37)], 'video8', 5),
    (255, [(9, 90)], 'video3', 5), (256, [(2, 300)], 'randn0.8', 5), (257, [(7, 1003)], 'video8', 30),
    (65, [(7, 1003), (1100, 16)], 'sparse_sel', 30), (33, [(7, 1003), (1100, 17)], 'video3', 30),
    (100, [(1, 460), (500, 1)], 'randn0.8', 30), (70, [(1, 460), (500, 17)], 'video8', 30), (129, [(17, 460)], 'cluster', 30),
    (65, [(0, 640)], 'cluster_flat', 30), (257, [(0, 2000), (2100, 1620), (4000, 1397)], 'video3', 30),
]
# pass 1 of one form is fed with the maxima and the threshold of ANOTHER form's pass 0; (nq4 -> nq2dma) is what MemoryManager._affinity_batch runs
PAIRS = [('nq4', 'nq2dma'), ('nq2dma', 'nq1'), ('nq1', 'nq2'), ('nq2', 'nq4')]


def test_the_score_cases_reach_every_size():
    assert {c[0] for c in SCORE_CASES} >= {1, 63, 64, 65, 127, 128, 129, 255, 256, 257}
    G = lambda r: sum(-(-n // 16) for _, n in r)
    assert {G(c[1]) for c in SCORE_CASES} >= {1, 3, 4, 5, 8, 9, 63, 64, 65, 29, 30, 31, 19} and {len(c[1]) for c in SCORE_CASES} == {1, 2, 3}
    assert {c[2] for c in SCORE_CASES} == set(A.REGIMES) and any(4900 < sum(n for _, n in c[1]) < 5100 for c in SCORE_CASES)
    assert {n for c in SCORE_CASES for _, n in c[1]} >= {1, 15, 16, 17, 37, 1003} and all(s % 16 for c in SCORE_CASES[:15] for s, _ in c[1][:1])


@pytest.mark.parametrize('HW,ranges,regime,top_k', SCORE_CASES)
def test_score_passes(HW, ranges, regime, top_k):
    c = A.AffCase(DEV, HW=HW, ranges=ranges, regime=regime, seed=HW + len(ranges), top_k=top_k)
    ol = O.OpList()
    c.prep(ol)
    p0 = {f: c.passes(f) for f in FORMS}
    for f in FORMS:
        c.score0(ol, p0[f], f)
        c.select(ol, p0[f])
    runs = {}
    for src, form in PAIRS:
        for skip in (True, False):
            tag = f'{src}>{form}{"+skip" if skip else ""}'
            b = c.b
            lists = dict(p0[src], cval=b.output('cval' + tag, (c.HWp, c.cap), F32), cidx=b.output('cidx' + tag, (c.HWp, c.cap), I32),
                         count=b.output('count' + tag, (c.HWp * A.AFF_CSTRIDE,), I32))
            c.select(ol, lists)                                                  # (the same tau again: this launch clears the new counters)
            c.score1(ol, lists, form, skip=skip)
            runs[tag] = lists
    ex, arr = launch(ol)
    sref = c.score_ref()
    what = f'{regime} HW={HW} G={c.G}'
    if regime == 'cluster_flat':
        must, _ = A.candidates_ref(sref['S'], sref['bound'], A.select_ref(A.tile_max_ref(sref['S'], sref['bound'], c.ranges)[0].float(), top_k))
        assert int(must[:16].sum()) > A.AFF_WCAP                                # one wave's list overflows: the flush-and-restart path runs
    r0 = {f: A.verify_score0(c, p0[f], sref=sref) for f in FORMS}
    for f in FORMS:
        A.verify_select(c, p0[f])
        assert torch.equal(A.bits(p0[f]['gmax'][:HW, :c.G]), A.bits(p0[FORMS[0]]['gmax'][:HW, :c.G])), (what, f, 'pass-0 maxima differ between forms')
    r1, V = {}, {}
    for tag, lists in runs.items():
        r1[tag], V[tag] = A.verify_score1(c, lists, sref=sref, what=f'{what} {tag}')
    first = next(iter(V))
    for tag in V:
        assert A.same_where_both(V[tag], V[first]), (what, tag, 'a candidate value differs between forms')
        assert torch.equal(torch.isnan(V[tag]), torch.isnan(V[first])), (what, tag, 'the candidate SETS differ between forms')
    assert c.b.guards_intact()
    first_V = V
    rerun_is_identical(c.b, ex, arr, skip=('cval', 'cidx'))
    for tag, lists in runs.items():                                              # the lists of the second run: the same sets with the same values
        _, V2 = A.verify_score1(c, lists, sref=sref, what=f'{what} {tag} (second run)')
        assert torch.equal(A.bits(V2), A.bits(first_V[tag]))
    print('aff_ref64 ratio score', what, f'gmax={max(r0.values()):.3g} cand={max(r1.values()):.3g}',
          f'lists={int(min(c.counts(l).min() for l in runs.values()))}..{int(max(c.counts(l).max() for l in runs.values()))}')


def test_score_stacked_frames_match_their_one_frame_launches():
    """frames = 3 at 128 rows per frame, HW = 100: rows 100..127 of every frame stay silent, every frame equals its own one-frame launch in
    set and in value bits (pass 0 on nq4, pass 1 on nq2dma: the product's pairing)."""
    HW, ranges, F_ = 100, [(3, 300), (400, 37)], 3
    c = A.AffCase(DEV, HW=HW, ranges=ranges, regime='video3', seed=3, top_k=30, frames=F_, HWp=128)
    ol = O.OpList()
    c.prep(ol)
    p = c.passes('s')
    c.score0(ol, p, 'nq4')
    c.select(ol, p)
    c.score1(ol, p, 'nq2dma')
    ones = []
    for f in range(F_):
        c1 = A.AffCase(DEV, HW=HW, ranges=ranges, top_k=30, HWp=128, keys=(c.mkey, c.mshr, c.qkey[f:f + 1], c.qsel[f:f + 1]))
        c1.prep(ol)
        p1 = c1.passes('o')
        c1.score0(ol, p1, 'nq2')
        c1.select(ol, p1)
        c1.score1(ol, p1, 'nq2')
        ones.append((c1, p1))
    launch(ol)
    worst = 0.0
    for f, (c1, p1) in enumerate(ones):
        sref = c.score_ref(f)
        worst = max(worst, A.verify_score0(c, p, f, sref=sref))
        A.verify_select(c, p, f)
        r, V = A.verify_score1(c, p, f, sref=sref, what=f'stacked frame {f}')
        _, V1 = A.verify_score1(c1, p1, what=f'one frame {f}')
        assert torch.equal(A.bits(c.frame_rows(p['gmax'], f)[:, :c.G]), A.bits(p1['gmax'][:HW, :c.G]))
        assert torch.equal(A.bits(c.frame_rows(p['tau'], f)), A.bits(p1['tau'][:HW])) and torch.equal(A.bits(V), A.bits(V1))
        assert c1.b.guards_intact()
        worst = max(worst, r)
    assert c.b.guards_intact()
    print(f'aff_ref64 ratio score stacked={worst:.3g}')


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('tiles', [4, 8, 12])
def test_score_tiles_per_block_override(form, tiles):
    """i[13] (tuning override: tiles per block): 19 tiles are 5 groups, in block rows of 1 | 2 and 1 | 3 and 2 groups -- the same bits as the
    launcher's own split."""
    c = A.AffCase(DEV, HW=129, ranges=[(2, 300)], regime='video3', seed=2, top_k=5)
    ol = O.OpList()
    c.prep(ol)
    p, q = c.passes('d'), c.passes('o')
    c.score0(ol, p, form)
    c.select(ol, p)
    c.score1(ol, p, form)
    k0 = c.score0(ol, q, form)
    c.select(ol, q)
    for k in (k0, c.score1(ol, q, form)):
        ol.recs[k][2][13] = tiles
    launch(ol)
    sref = c.score_ref()
    A.verify_score0(c, q, sref=sref)
    A.verify_select(c, q)
    _, V = A.verify_score1(c, p, sref=sref)
    _, Vq = A.verify_score1(c, q, sref=sref, what=f'tiles per block {tiles}')
    assert torch.equal(A.bits(q['gmax'][:c.HW, :c.G]), A.bits(p['gmax'][:c.HW, :c.G])) and torch.equal(A.bits(V), A.bits(Vq)) and c.b.guards_intact()


@pytest.mark.parametrize('form', ['nq2', 'nq2dma'])
def test_score_bank_table_form_matches_the_per_bank_one_frame_launches(form):
    """flags&4: four stacked frames over two banks (frame f reads bank f % 2 through the table), against the float64 reference of that bank's
    operands and against one-frame launches on that bank: the same maxima, thresholds, candidate sets and value bits."""
    HW, HWp, F_, ranges = 100, 128, 4, [(3, 300), (400, 37)]
    c = A.AffCase(DEV, HW=HW, ranges=ranges, regime='video3', seed=5, top_k=30, frames=F_, HWp=HWp)
    other = A.AffCase(DEV, HW=HW, ranges=ranges, regime='randn0.8', seed=6, top_k=30, HWp=HWp)           # its memory side is bank 1
    banks = [c, other]
    table = c.b.operand(torch.tensor([[x.Ahi.data_ptr(), x.Alo.data_ptr(), x.scale.data_ptr()] for x in banks], dtype=I64))
    ol = O.OpList()
    c.prep(ol)
    other.prep(ol)
    p = c.passes('t')
    c.score0(ol, p, form, banks=(table, 2))
    c.select(ol, p)
    c.score1(ol, p, form, banks=(table, 2))
    ones = []
    for f in range(F_):
        bk, r0, b = banks[f % 2], f * HWp, c.b
        gb = b.output(f'g1{f}', (HWp * c.Gld + HWp,), F32)
        o = dict(gmax=gb[:HWp * c.Gld].view(HWp, c.Gld), tau=gb[HWp * c.Gld:], cval=b.output(f'cv1{f}', (HWp, c.cap), F32),
                 cidx=b.output(f'ci1{f}', (HWp, c.cap), I32), count=b.output(f'cn1{f}', (HWp * A.AFF_CSTRIDE,), I32))
        args = (bk.Ahi, bk.Alo, bk.scale, c.Bhi[r0:r0 + HWp], c.Blo[r0:r0 + HWp], c.cq[r0:r0 + HWp])
        kw = dict(HW=HW, HWp=HWp, ranges=c.ranges, cap=c.cap, nq=2)
        ol.aff_score(*args, o['gmax'], None, None, None, mode=0, **kw)
        ol.aff_select(o['gmax'], o['tau'], HW=HW, HWp=HWp, G=c.G, top_k=30, clear_count=o['count'])
        ol.aff_score(*args, o['tau'], o['cval'], o['cidx'], o['count'], mode=1, gmax_precedes_tau=True, **kw)
        ones.append(o)
    launch(ol)
    worst = 0.0
    for f, o in enumerate(ones):
        bk, r0 = banks[f % 2], f * HWp
        sref = A.score_ref(bk.Ahi, bk.Alo, bk.scale, c.Bhi[r0:], c.Blo[r0:], c.cq[r0:], c.ranges, HW)
        worst = max(worst, A.verify_score0(c, p, f, sref=sref))
        A.verify_select(c, p, f)
        r, V = A.verify_score1(c, p, f, sref=sref, what=f'bank table frame {f}')
        _, V1 = A.check_candidates(o['cval'][:HW], o['cidx'][:HW], o['count'].view(-1, A.AFF_CSTRIDE)[:HW, 0], S=sref['S'], bound=sref['bound'], tau=o['tau'][:HW],
                                   ranges=c.ranges, gmax=o['gmax'][:HW], top_k=30, cap=c.cap, sent_v=A.SENT_F, sent_i=A.SENT_I, what=f'one frame {f}')
        assert torch.equal(A.bits(c.frame_rows(p['gmax'], f)[:, :c.G]), A.bits(o['gmax'][:HW, :c.G]))
        assert torch.equal(A.bits(c.frame_rows(p['tau'], f)), A.bits(o['tau'][:HW])) and torch.equal(A.bits(V), A.bits(V1))
        worst = max(worst, r)
    assert c.b.guards_intact() and other.b.guards_intact()
    print(f'aff_ref64 ratio score bank table {form}={worst:.3g}')


# ---- AFF_SELECT alone -------------------------------------------------------------------------------------------------------------------
K_SEL = 30


def _select_rows(g, rows, G, k):
    """Rows of tile maxima with what a selection gets wrong: runs of -inf, +-0, denormals, the k-th value repeated across the cut, an
    all-equal row, a strictly descending and an ascending one."""
    out = torch.randn((rows, G), generator=g) * 4
    for r in range(rows):
        kind = (r + G) % 6
        if kind == 0 and G > 3:
            out[r, G // 3:G // 3 + max(1, G // 2)] = A.NEG_INF
        elif kind == 1:
            sm = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 2.0 ** -126])
            out[r] = sm[torch.randint(0, 7, (G,), generator=g)]
        elif kind == 2 and G >= k:
            v = torch.sort(out[r], descending=True).values
            v[max(0, k - 4):min(G, k + 5)] = v[k - 1]
            out[r] = v[torch.randperm(G, generator=g)]
        elif kind == 3:
            out[r] = -7.25
        elif kind == 4:
            out[r] = -torch.arange(G, dtype=F32) * 0.5
        elif kind == 5:
            out[r] = torch.arange(G, dtype=F32) * 0.25 - 100
    return out


@pytest.mark.parametrize('G,coarse', [(G, 0) for G in (1, K_SEL - 1, K_SEL, K_SEL + 1, 255, 256, 257, 2000, 4095, 4096, 4097, 5000)] +
                         [(256, 2), (2000, 2), (4095, 2)])
def test_select_alone(G, coarse, monkeypatch):
    """Every values-per-lane step, the three coarse sizes (flags&2) and the radix kernel above 4096 tiles; the side jobs: counters cleared at
    stride AFF_CSTRIDE only, the life ranges advanced by exactly one over exactly nA / nB entries, or range A cleared (zero=)."""
    monkeypatch.setattr(O, 'SELECT_COARSE', coarse)
    g = torch.Generator().manual_seed(G)
    Gld = -(-G // 64) * 64
    for HW in (1, 4, 5, 9):
        b = A.Bufs(DEV)
        vals = _select_rows(g, HW, G, K_SEL)
        gm = torch.full((HW, Gld), float('nan'))
        gm[:, :G] = vals
        gmax, tau = b.operand(gm), b.output('tau', (HW,), F32)
        count = b.output('count', (HW * A.AFF_CSTRIDE,), I32)
        nA, nB = 37, 5
        lifeA, lifeB = b.output('lifeA', (nA + 9,), F32, torch.arange(nA + 9.0)), b.output('lifeB', (nB + 9,), F32, torch.arange(nB + 9.0))
        zero = b.output('zero', (nA + 9,), F32, torch.arange(nA + 9.0) + 1)
        tau2 = b.output('tau2', (HW,), F32)
        ol = O.OpList()
        ol.aff_select(gmax, tau, HW=HW, HWp=64, G=G, top_k=K_SEL, clear_count=count, ticks=[(lifeA, nA), (lifeB, nB)])
        ol.aff_select(gmax, tau2, HW=HW, HWp=64, G=G, top_k=K_SEL, zero=(zero, nA))
        ex, arr = launch(ol)
        want = A.select_ref(vals, K_SEL)
        for t in (tau, tau2):
            assert bool((t.cpu() == want).all()), (G, HW, t.cpu(), want)
        cnt = count.view(HW, A.AFF_CSTRIDE).cpu()
        assert bool((cnt[:, 0] == 0).all()) and bool((cnt[:, 1:] == A.SENT_I).all())
        for life, n in ((lifeA, nA), (lifeB, nB)):
            assert torch.equal(life.cpu(), torch.arange(n + 9.0) + (torch.arange(n + 9) < n).float())
        assert torch.equal(zero.cpu(), torch.where(torch.arange(nA + 9) < nA, torch.zeros(()), torch.arange(nA + 9.0) + 1))
        assert b.guards_intact()


@pytest.mark.parametrize('G', [K_SEL, 300, 4100])
def test_select_stacked_frames_leave_the_padding_rows_alone(G):
    F_, HWp, HW = 3, 64, 37
    g = torch.Generator().manual_seed(G)
    Gld = -(-G // 64) * 64
    b = A.Bufs(DEV)
    gm = torch.full((F_ * HWp, Gld), float('nan'))
    gm[:, :G] = _select_rows(g, F_ * HWp, G, K_SEL)
    tau, count = b.output('tau', (F_ * HWp,), F32), b.output('count', (F_ * HWp * A.AFF_CSTRIDE,), I32)
    ol = O.OpList()
    ol.aff_select(b.operand(gm), tau, HW=HW, HWp=HWp, G=G, top_k=K_SEL, clear_count=count, frames=F_)
    launch(ol)
    t, want = tau.cpu().view(F_, HWp), A.select_ref(gm[:, :G], K_SEL).view(F_, HWp)
    assert bool((t[:, :HW] == want[:, :HW]).all()) and bool((t[:, HW:] == A.SENT_F).all())
    cnt = count.view(F_ * HWp, A.AFF_CSTRIDE).cpu()
    assert bool((cnt[:, 0] == 0).all()) and bool((cnt[:, 1:] == A.SENT_I).all()) and b.guards_intact()


# ---- AFF_READOUT alone, on hand-built lists -------------------------------------------------------------------------------------------
def _readout_case(R, top_k, K, CV, cap=1024, nslots=2000, frames=1, HWp=None):
    return A.AffCase(DEV, HW=R, ranges=[(0, nslots - 3)], seed=top_k + K, top_k=top_k, K=K, CV=CV, cap=cap, frames=frames, HWp=HWp)


def _put_lists(c, p, cv, ci, cnt, f=0):
    r0, R = f * c.HWp, cnt.numel()
    p['cval'][r0:r0 + R].copy_(cv)
    p['cidx'][r0:r0 + R].copy_(ci)
    p['count'].view(-1, A.AFF_CSTRIDE)[r0:r0 + R, 0] = cnt.to(DEV)
    for n in ('cval', 'cidx', 'count'):                                          # (these are inputs here: what `reset` restores)
        name = [k for k, (v, _) in c.b.outs.items() if v.data_ptr() == p[n].data_ptr()][0]
        c.b.outs[name] = (p[n], p[n].clone())


@pytest.mark.parametrize('top_k,K,CV', [(1, 1, 256), (5, 3, 256), (30, 5, 256), (64, 1, 256), (30, 3, 8)])
def test_readout_hand_built_lists(top_k, K, CV):
    cv, ci, cnt, groups = A.hand_lists(top_k, 1024, 1997, seed=top_k)
    R = cnt.numel()
    c = _readout_case(R, top_k, K, CV)
    p = c.passes('h')
    _put_lists(c, p, cv, ci, cnt)
    ol = O.OpList()
    y, use, ovf = c.readout(ol, p, 'fx', usage_fx=True)
    y2, use2, ovf2 = c.readout(ol, p, 'f32', usage_fx=False)
    ex, arr = launch(ol)
    what = f'readout top_k={top_k} K={K} CV={CV}'
    ry, ru = A.verify_readout(c, p, y, use, ovf, what=what + ' fx')
    ry2, ru2 = A.verify_readout(c, p, y2, use2, ovf2, what=what + ' f32')
    assert torch.equal(A.bits(y), A.bits(y2))
    empty = (cnt == 0).nonzero().flatten()
    assert bool((y[0][:, empty].float() == 0).all())                             # cnt == 0: y == 0 exactly
    for grp in groups:                                                           # the same list in another order: the same bits
        for r in grp[1:]:
            assert torch.equal(A.bits(y[0][:, r]), A.bits(y[0][:, grp[0]])), (what, 'the result depends on the order of the list', grp)
    assert c.b.guards_intact()
    rerun_is_identical(c.b, ex, arr, skip=('usef32',))
    print('aff_ref64 ratio', what, f'y={max(ry, ry2):.3g} usage_fx={ru:.3g} usage_f32={ru2:.3g}')


@pytest.mark.parametrize('kw,msg', [(dict(top_k=65), 'top_k'), (dict(CV=12), 'CV'), (dict(cap=1022), 'cap')])
def test_readout_refuses_what_it_cannot_run(kw, msg):
    args = dict(top_k=30, K=1, CV=256, cap=1024)
    args.update(kw)
    c = A.AffCase(DEV, HW=4, ranges=[(0, 100)], top_k=args['top_k'], K=1, CV=args['CV'] if args['CV'] % 8 == 0 else 16, cap=args['cap'])
    c.CV = args['CV']
    p = c.passes('r')
    p['count'].zero_()
    ol = O.OpList()
    y = c.b.output('y', (1, 1, 4, 16), BF16)
    use, ovf = c.b.output('use', (c.nslots,), I64, 0), c.b.output('ovf', (1,), I32, 0)
    ol.aff_readout(p['cval'], p['cidx'], p['count'], c.vptrs, use, y, ovf, HW=4, cap=c.cap, top_k=c.top_k, K=1, CV=c.CV, usage_fx=True)
    with pytest.raises(RuntimeError, match='aff_readout'):
        _lib.HipExecutor().run(ol.finalize())
    torch.cuda.synchronize()
    assert bool((y == A.SENT_F).all()) and int(ovf) == 0 and c.b.guards_intact()        # nothing launched


def test_readout_overflowing_lists():
    """count = cap + 5: the overflow counter takes one per such query, the list is cut to cap entries and y stays finite; with identical value
    rows y is that row within the bound whatever was selected (the selected set is not determinate there: nothing more is asserted)."""
    top_k, cap, R = 30, 1024, 3
    c = _readout_case(R, top_k, 2, 256)
    row = c.d_values[0][5].clone()
    for v, d in zip(c.values, c.d_values):
        d[:1997] = row
        v[:1997] = row.cpu()
    g = torch.Generator().manual_seed(1)
    cv = torch.randn((R, cap), generator=g)
    ci = torch.stack([torch.randperm(1997, generator=g)[:cap] for _ in range(R)]).to(I32)
    p = c.passes('o')
    _put_lists(c, p, cv, ci, torch.tensor([cap + 5, cap, cap + 5], dtype=I32))
    ol = O.OpList()
    y, use, ovf = c.readout(ol, p, 'fx')
    launch(ol)
    assert int(ovf) == 2 and bool(torch.isfinite(y.float()).all())
    want = row.cpu().double()[None, None].expand(2, R, 256)
    e = (A.gamma(128) + 64 * 1e-5) * want.abs() + 128 * A.FTZ                          # weights sum to one within 64 x their own bound (< 1e-5 each)
    A.check_bound(y[0].cpu().reshape(-1, 256), want.reshape(-1, 256), (e + A.U_BF16 * (want.abs() + e)).reshape(-1, 256), what='overflow y')
    assert c.b.guards_intact()


@pytest.mark.parametrize('nrows', [1, 7, 8, 9, 63, 65])
def test_readout_xcd_striping_writes_every_query_once(nrows):
    """Block b serves query (b & 7) * per + (b >> 3): every real query is written (y starts as NaN) and nothing else is."""
    top_k = 5
    c = _readout_case(nrows, top_k, 1, 8, nslots=300)
    g = torch.Generator().manual_seed(nrows)
    cv = torch.full((nrows, c.cap), A.SENT_F)
    ci = torch.full((nrows, c.cap), A.SENT_I, dtype=I32)
    cv[:, :9] = torch.randn((nrows, 9), generator=g)
    ci[:, :9] = torch.stack([torch.randperm(297, generator=g)[:9] for _ in range(nrows)]).to(I32)
    p = c.passes('x')
    _put_lists(c, p, cv, ci, torch.full((nrows,), 9, dtype=I32))
    ol = O.OpList()
    y, use, ovf = c.readout(ol, p, 'fx')
    launch(ol)
    A.verify_readout(c, p, y, use, ovf, what=f'striping nrows={nrows}')
    assert abs(float(A.usage_float(use).sum()) - nrows) < 1e-4 and c.b.guards_intact()


def test_readout_stacked_frames_and_fixed_point_usage_by_block_order():
    """frames = 2 with usage_stride: the stacked launch against the frames one by one -- two different block orders, the same fixed-point
    counters bit for bit, the same y."""
    top_k, HW, HWp = 30, 37, 64
    c = _readout_case(HW, top_k, 2, 256, frames=2, HWp=HWp)
    p = c.passes('s')
    p['count'].view(-1, A.AFF_CSTRIDE)[HW:HWp, 0] = 7                                  # (a padding row's counter is never looked at)
    for f in range(2):
        cv, ci, cnt, _ = A.hand_lists(top_k, 1024, 1997, seed=10 + f)
        _put_lists(c, p, cv[:HW], ci[:HW], cnt[:HW], f)
    ol = O.OpList()
    y, use, ovf = c.readout(ol, p, 'st')
    y1 = c.b.output('y1', (2, c.K, HW, c.CV), BF16, float('nan'))
    use1 = c.b.output('use1', (2, c.nslots), I64, 0)
    for f in range(2):
        r0 = f * HWp
        ol.aff_readout(p['cval'][r0:], p['cidx'][r0:], p['count'][r0 * A.AFF_CSTRIDE:], c.vptrs, use1[f], y1[f], ovf, HW=HW, cap=c.cap, top_k=top_k,
                       K=c.K, CV=c.CV, usage_fx=True)
    ex, arr = launch(ol)
    for f in range(2):
        A.verify_readout(c, p, y, use, ovf, f, what=f'stacked read-out frame {f}')
    assert torch.equal(A.bits(y), A.bits(y1)) and torch.equal(use, use1) and c.b.guards_intact()
    rerun_is_identical(c.b, ex, arr)


# ---- the chain, end to end, against the truth from the raw keys --------------------------------------------------------------------------
def _logit_errors(c, p, f, ref):
    """Signed logit errors on every query's true top-k: the kernel's (from cand_val) and the dense fp32 reference algorithm's."""
    sl, S = ref['slots'], ref['S']
    lut = torch.full((int(sl.max()) + 1,), -1, dtype=torch.int64)
    lut[sl] = torch.arange(sl.numel())
    sim32 = get_similarity(c.mkey[sl].t().float(), c.mshr[sl].float(), c.qkey[f].t().float(), c.qsel[f].t().float()).t().double()
    cv, ci, cnt = c.frame_rows(p['cval'], f).cpu(), c.frame_rows(p['cidx'], f).cpu(), c.counts(p, f).cpu()
    out = dict(kernel=[0.0, 0.0], fp32=[0.0, 0.0])
    for j in range(c.HW):
        top = ref['top'][j]
        Sk = torch.full((sl.numel(),), float('nan'), dtype=torch.float64)
        n = int(cnt[j])
        Sk[lut[ci[j, :n].long()]] = cv[j, :n].double()
        for name, Si in (('kernel', Sk), ('fp32', sim32[j])):
            d = (Si - S[j])[top]
            d = d[~torch.isnan(d)]
            if d.numel():
                out[name][0] = max(out[name][0], float(d.abs().max()))
                out[name][1] = max(out[name][1], float(torch.expm1(d.max() - d.min())))
    return out


@pytest.mark.parametrize('frames', [1, 3])
@pytest.mark.parametrize('regime,seed', A.CHAIN_CASES)
def test_chain_against_the_truth(regime, seed, frames):
    """The product's launch sequence: one frame on the default form, three stacked frames on nq4 (pass 0) and nq2dma (pass 1).  Prints the
    kernel's and the fp32 reference algorithm's worst logit error and the relative softmax-weight error that follows: findings, not thresholds."""
    c = A.AffCase(DEV, HW=A.CHAIN_HW, ranges=A.CHAIN_RANGES, regime=regime, seed=seed, K=3, top_k=30, frames=frames)
    assert c.nslots == A.CHAIN_NSLOTS
    refs = [A.pipeline_ref(c.mkey, c.mshr, c.qkey[f], c.qsel[f], c.ranges, c.values, 30, c.nslots) for f in range(frames)]
    for ref in refs:                                                             # the cap, from the reference alone, before any kernel output
        assert float(ref['ambiguous'].float().mean()) <= A.AMBIG_CAP
    ol = O.OpList()
    c.prep(ol)
    p = c.passes('c')
    f0, f1 = ('nq2', 'nq2') if frames == 1 else ('nq4', 'nq2dma')
    c.score0(ol, p, f0)
    c.select(ol, p)
    c.score1(ol, p, f1)
    y, use, ovf = c.readout(ol, p, 'c')
    ex, arr = launch(ol)
    assert int(ovf) == 0
    for f, ref in enumerate(refs):
        ok = ~ref['ambiguous']
        got = y[f].cpu().double()
        ry = A.check_bound(got[:, ok].reshape(-1, c.CV), ref['y'][:, ok].reshape(-1, c.CV), ref['ybound'][:, ok].reshape(-1, c.CV), what=f'chain y {regime} f={f}')
        ru = A.check_bound(A.usage_float(use[f]).view(-1, 1), ref['usage'].view(-1, 1), ref['ubound'].view(-1, 1) + 1e-30, what=f'chain usage {regime} f={f}')
        sref = c.score_ref(f)
        r0 = A.verify_score0(c, p, f, sref=sref)
        A.verify_select(c, p, f)
        r1, _ = A.verify_score1(c, p, f, sref=sref, what=f'chain {regime} f={f}')
        ryl, rul = A.verify_readout(c, p, y, use, ovf, f, what=f'chain {regime} f={f}')
        le = _logit_errors(c, p, f, ref)
        print(f'aff_ref64 chain {regime} frames={frames} f={f} ambiguous={int(ref["ambiguous"].sum())}/{c.HW} ratio: gmax={r0:.3g} cand={r1:.3g} readout_y={ryl:.3g} '
              f'readout_usage={rul:.3g} chain_y={ry:.3g} chain_usage={ru:.3g} | logit error: kernel={le["kernel"][0]:.3g} fp32={le["fp32"][0]:.3g} '
              f'(true top score bound {float(ref["E"].max()):.3g}) | relative weight error: kernel={le["kernel"][1]:.3g} fp32={le["fp32"][1]:.3g}')
    assert c.b.guards_intact()
    rerun_is_identical(c.b, ex, arr, skip=('cval', 'cidx'))
