"""The kernels that write the memory (csrc/bank.hip; BANK_WRITE, USAGE_TICK, AXPY, COPY2D, MEMSET32, CAST, SUMMARIZE, ADD_PE of
csrc/elementwise.hip) on the MI355X against the float64 / exact references of tests/bank_ref64.py, stage by stage and element by element:
the shared case list, one small launch sequence per case, outputs pre-filled with NaN or sentinel words between sentinel elements that must
survive, every value within its derived bound, every exact property asserted by bits, and a second run of the same launches bit-identical in
EVERY output (nothing here uses float atomics; the column maxima are integer atomics on order-preserving keys).  Each test prints its worst
|err| / bound per stage and regime; DESIGN.md keeps the tables."""
import pytest
import torch

import bank_ref64 as B
from cutie_amd import _lib
from cutie_amd import ops as O
from oracle.net import get_similarity

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, BF16, I32, I64 = torch.float32, torch.bfloat16, torch.int32, torch.int64


def execute(ol, b):
    """Run, then run the same launches again from the same initial buffers: the same bits in every output."""
    ex, arr = _lib.HipExecutor(), ol.finalize()
    ex.run(arr)
    torch.cuda.synchronize()
    first = b.snapshot()
    assert b.guards_intact()
    b.reset()
    ex.run(arr)
    torch.cuda.synchronize()
    for n, t in first.items():
        assert torch.equal(B.bits(b[n]), B.bits(t)), (n, 'a second run of the same launches differs')


def once(ol, b=None):
    _lib.HipExecutor().run(ol.finalize())
    torch.cuda.synchronize()


# ---- the shared case list ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,k,kind,nzero', B.RANK_CASES)
def test_rank_select_gather(n, k, kind, nzero):
    B.run_rank_case(DEV, execute, n, k, kind, nzero)


@pytest.mark.parametrize('n,P,regime', B.AFF_CASES)
def test_consol_aff(n, P, regime):
    r, _ = B.run_aff_case(DEV, execute, n, P, regime)
    print(f'bank_ref64 ratio consol_aff {regime} n={n} P={P} S={r["S"]:.3g}')


@pytest.mark.parametrize('n,P,C,K,skind,vkind,adjacent', B.READ_CASES)
def test_consol_read(n, P, C, K, skind, vkind, adjacent):
    r, _ = B.run_read_case(DEV, execute, n, P, C, K, skind, vkind, adjacent)
    print(f'bank_ref64 ratio consol_read {skind}/{vkind} n={n} P={P} C={C} K={K} y={r["y"]:.3g} out_shr={r["out_shr"]:.3g}')


@pytest.mark.parametrize('n,P,K,regime,seed,keep', B.CHAIN_CASES)
def test_chain_as_compress_issues_it(n, P, K, regime, seed, keep):
    r = B.run_chain_case(DEV, execute, n, P, K, regime, seed, keep)
    print(f'bank_ref64 ratio chain {regime} n={n} P={P} K={K} ' + ' '.join(f'{k}={v:.3g}' for k, v in r.items()))


@pytest.mark.parametrize('case', B.TICK_CASES)
def test_usage_tick(case):
    B.run_tick_case(DEV, execute, *case)


@pytest.mark.parametrize('words', B.BW_LAUNCHES)
def test_bank_write(words):
    B.run_bank_write_case(DEV, execute, words)


@pytest.mark.parametrize('n', [1, 255, 256, 257, 1000])
def test_copy_fill_cast_axpy(n):
    B.run_misc_case(DEV, execute, n)


@pytest.mark.parametrize('K,HW,C,regime,f32_form', B.SUM_CASES)
def test_summarize(K, HW, C, regime, f32_form):
    r = B.run_summarize_case(DEV, execute, K, HW, C, regime, f32_form, partials=True)
    print(f'bank_ref64 ratio summarize {regime} K={K} HW={HW} C={C} f32={f32_form} y={r:.3g}')


@pytest.mark.parametrize('Bn,n8', [(1, 1), (3, 1), (1, 300), (3, 333)])
def test_add_pe(Bn, n8):
    r = B.run_add_pe_case(DEV, execute, Bn, n8)
    print(f'bank_ref64 ratio add_pe B={Bn} n8={n8} y={r:.3g}')


# ---- bit-identities the code promises ---------------------------------------------------------------------------------------------------
def _read_setup(b, n, P, regime, seed):
    c = B.make_consol(seed, regime, n, P)
    pk, pe, _ = B.pick_prototypes(c, P)
    S, colmax, ldS = B.aff_buffers(b, n, P)
    ol = O.OpList()
    d_shr = b.operand(c['cshr'])
    ol.consol_aff(b.operand(c['ckey']), d_shr, b.operand(pk), b.operand(pe), S, colmax, n=n, P=P)
    return c, ol, S, colmax, d_shr


def test_consol_read_of_K_objects_equals_K_launches_of_one():
    n, P, C, K = 513, 17, 256, 3
    b = B.Bufs(DEV)
    c, ol, S, colmax, d_shr = _read_setup(b, n, P, 'video3', 11)
    rc = B.ReadCase(DEV, b, n, P, C, K, 'randn', True, 21)
    rc.launch(ol, S, colmax, d_shr)
    singles = []
    for o in range(K):
        bank = b.output(f'single{o}', tuple(rc.before[o].shape), BF16, rc.before[o])
        vp = b.operand(torch.tensor([bank.data_ptr()], dtype=I64))
        osh = b.output(f'single_shr{o}', (P + 2,), F32)
        ol.consol_read(S, colmax, vp, d_shr, b.output(f'single_part{o}', (O.OpList.consol_scratch_floats(n, P, C, 1),), F32), osh, n=n, P=P, C=C, K=1, src=rc.src, dst=rc.dst)
        singles.append((bank, osh))
    execute(ol, b)
    for o, (bank, osh) in enumerate(singles):
        assert B.same_bits(bank, rc.banks[o]) and B.same_bits(osh, rc.out_shr), (o, 'K objects in one launch differ from one launch per object')
    assert b.guards_intact()


def test_a_prototype_does_not_depend_on_the_launch_that_carried_it():
    """P = 136 is two p0 launches (128 + 8); the first 128 prototypes alone are one: the same bits."""
    n, C, K = 300, 128, 2
    b = B.Bufs(DEV)
    c, ol, S, colmax, d_shr = _read_setup(b, n, 136, 'video8', 12)
    rc = B.ReadCase(DEV, b, n, 136, C, K, 'x64', False, 22)
    rc.launch(ol, S, colmax, d_shr)
    banks = [b.output(f'first{o}', tuple(rc.before[o].shape), BF16, rc.before[o]) for o in range(K)]
    vp = b.operand(torch.tensor([v.data_ptr() for v in banks], dtype=I64))
    osh = b.output('first_shr', (130,), F32)
    ol.consol_read(S, colmax, vp, d_shr, b.output('first_part', (O.OpList.consol_scratch_floats(n, 128, C, K),), F32), osh, n=n, P=128, C=C, K=K, src=rc.src, dst=rc.dst)
    execute(ol, b)
    for o in range(K):
        assert B.same_bits(banks[o][rc.dst:rc.dst + 128], rc.banks[o][rc.dst:rc.dst + 128])
        assert B.same_bits(banks[o][rc.dst + 128:], rc.before[o][rc.dst + 128:])
    assert B.same_bits(osh[:128], rc.out_shr[:128]) and b.guards_intact()


# ---- refusals: the launcher returns -2 with a message before any kernel starts -----------------------------------------------------------
def _refused(ol, b, match, outs):
    ex, arr = _lib.HipExecutor(), ol.finalize()
    rc = ex.lib.cutie_exec(arr.ctypes.data, len(arr), ex.stream())
    assert rc == -2, rc
    assert match in ex.lib.cutie_hip_last_error().decode()
    with pytest.raises(RuntimeError, match=match):
        ex.run(arr)
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == (B.SENT_F if t.is_floating_point() else B.SENT_I)).all()), 'a refused launch wrote something'
    assert b.guards_intact()


@pytest.mark.parametrize('what', ['scratch', 'row', 'k>n', 'n<1'])
def test_rank_select_refuses(what):
    n, k = 40, 8
    b = B.Bufs(DEV)
    use, life = B.make_usage(1, 'random', n)
    order, side, scratch = b.output('order', (k,), I32), b.output('side', (k, 4), I32), b.output('scratch', (16 * n,), I32)
    src = b.operand(torch.zeros((n, 4), dtype=I32))
    ol = O.OpList()
    idx = ol.rank_select(b.operand(use), b.operand(life), order, n=n, k=k, scratch=scratch, gathers=[(src, side, 16)])
    ints, ptrs = ol.recs[idx][2], ol.recs[idx][4]
    if what == 'scratch':
        ptrs[3] = 0
    elif what == 'row':
        ints[2] = 3
    elif what == 'k>n':
        ints[1] = n + 1
    else:
        ints[0], ints[1] = 0, 0
    _refused(ol, b, 'rank_select', [order, side, scratch])


@pytest.mark.parametrize('ldS', [48, 32])
def test_consol_aff_refuses(ldS):
    n, P = 40, 4
    b = B.Bufs(DEV)
    c = B.make_consol(1, 'randn0.8', n, P)
    pk, pe, _ = B.pick_prototypes(c, P)
    S, colmax = b.output('S', (P, 64), F32), b.output('colmax', (P,), I32)
    ol = O.OpList()
    idx = ol.consol_aff(b.operand(c['ckey']), b.operand(c['cshr']), b.operand(pk), b.operand(pe), S, colmax, n=n, P=P)
    ol.recs[idx][2][2] = ldS
    _refused(ol, b, 'consol_aff', [S, colmax])


@pytest.mark.parametrize('what', ['C', 'K', 'ldS'])
def test_consol_read_refuses(what):
    n, P, C = 40, 4, 128
    b = B.Bufs(DEV)
    S0, cm0 = B.hand_S('ramp', n, P, 64)
    bank = b.output('bank', (n + P + 8, C), BF16)
    part, osh = b.output('part', (O.OpList.consol_scratch_floats(n, P, C, 1),), F32), b.output('osh', (P,), F32)
    ol = O.OpList()
    idx = ol.consol_read(b.operand(S0), b.operand(cm0), b.operand(torch.tensor([bank.data_ptr()], dtype=I64)), b.operand(torch.ones(n)), part, osh,
                         n=n, P=P, C=C, K=1, src=P + 4, dst=2)
    ints = ol.recs[idx][2]
    if what == 'C':
        ints[2] = 64
    elif what == 'K':
        ints[3] = 0
    else:
        ints[4] = 32
    _refused(ol, b, 'consol_read', [bank, part, osh])


@pytest.mark.parametrize('what', ['Q', 'C', 'scratch'])
def test_summarize_refuses(what):
    K, HW, C, Q = 1, 20, 64, 16
    feat, wl, m = B.make_summarize(1, 'plain', K, HW, C)
    b = B.Bufs(DEV)
    y, scratch = b.output('y', (K, Q, C + 1), F32), b.output('scratch', (K, 1, Q, C + 1), F32)
    ol = O.OpList()
    idx = ol.summarize(b.operand(feat.to(BF16)), b.operand(wl), b.operand(m), y, K=K, HW=HW, C=C, Q=Q, scratch=scratch)
    if what == 'Q':
        ol.recs[idx][2][3] = 8
    elif what == 'C':
        ol.recs[idx][2][2] = 32
    else:
        ol.recs[idx][4][4] = 0
    _refused(ol, b, 'summarize', [y, scratch])


def test_bank_write_refuses_a_negative_size():
    b = B.Bufs(DEV)
    dst, fill = b.output('dst', (16,), I32), b.output('fill', (16,), I32)
    ol = O.OpList()
    idx = ol.bank_write([(b.operand(torch.zeros(16, dtype=I32)), dst, 64)], [(fill, 16, 0)])
    ol.recs[idx][2][0] = -4
    _refused(ol, b, 'bank_write', [dst, fill])
    ol = O.OpList()
    idx = ol.bank_write([(b.operand(torch.zeros(16, dtype=I32)), dst, 64)], [(fill, 16, 0)])
    ol.recs[idx][2][6] = -1
    _refused(ol, b, 'bank_write', [dst, fill])


# ---- accuracy of the consolidation similarities: findings, not thresholds ------------------------------------------------------------------
@pytest.mark.parametrize('regime', ['randn0.8', 'video3', 'video8', 'sparse_sel'])
def test_accuracy_of_the_similarities_that_decide_the_softmax(regime):
    """Per regime: the worst |S - S_true| over each prototype's softmax-relevant candidates (within 20 of the column maximum) for the kernel and
    for oracle.net.get_similarity in fp32 on the same inputs, and the relative weight error e^(max d - min d) - 1 that follows.  Both expand the
    square; DESIGN.md keeps the table."""
    n, P = 1000, 128
    r, o = B.run_aff_case(DEV, once, n, P, regime, seed=77)
    c, true = o['c'], o['true']
    St = true['S']
    sim32 = get_similarity(c['ckey'].t().float(), c['cshr'].float(), o['pk'].t().float(), o['pe'].t().float()).t().double()
    rel = St >= St.max(1, keepdim=True).values - 20
    out = {}
    for name, Sx in (('kernel', o['S'][:P, :n].double()), ('fp32', sim32)):
        d = Sx - St
        hi = torch.where(rel, d, torch.full_like(d, -1e30)).max(1).values
        lo = torch.where(rel, d, torch.full_like(d, 1e30)).min(1).values
        out[name] = (float(d[rel].abs().max()), float(torch.expm1(hi - lo).max()))
    print(f'bank_ref64 accuracy {regime} n={n} P={P} relevant={int(rel.sum())} bound={float(true["bound"][rel].max()):.3g} ratio={r["S"]:.3g} | '
          f'|S - S_true|: kernel={out["kernel"][0]:.3g} fp32={out["fp32"][0]:.3g} | relative weight error: kernel={out["kernel"][1]:.3g} fp32={out["fp32"][1]:.3g}')
