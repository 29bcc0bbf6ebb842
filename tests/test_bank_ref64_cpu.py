"""tests/bank_ref64.py on the host: the float64 chain agrees with the reference algorithm (oracle's _consolidate: get_similarity,
topk_softmax, the v @ aff products) and SUMMARIZE with oracle.net's object_summarizer arithmetic, both evaluated in float64; the interpreter
(tests/mock_exec.py) passes every case of the shared list inside every bound and every exact check; no reference or bound is non-finite; and
the checks bite: each fault a memory-maintenance kernel can plausibly make is a knob of a float64 restatement of the stage (or a change of the
interpreter's outputs) -- with the knob off the restatement passes every case, with it on at least one check fails."""
import numpy as np
import pytest
import torch

import bank_ref64 as B
from cutie_amd import ops as O
from mock_exec import MockExecutor
from oracle.net import get_similarity, topk_softmax

F64, F32, BF16, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32


def mock(ol, b):
    MockExecutor().run(ol.finalize())


# ---- the references against the reference algorithm ----------------------------------------------------------------------------------
@pytest.mark.parametrize('regime', ['randn0.8', 'video3', 'video8', 'sparse_sel'])
def test_chain_ref_is_the_reference_consolidation_in_float64(regime):
    n, P, C = 300, 16, 32
    c = B.make_consol(5, regime, n, P)
    vals = [B.make_values(o, 'randn', n, C) for o in range(2)]
    ref = B.chain_ref(c, vals, P)
    usage = (c['use'] / c['life'])                                            # (fp32, as the reference divides)
    assert torch.unique(usage).numel() == n                                   # no tied quotients: topk's order is the stable sort's
    _, idx = torch.topk(usage, k=P, dim=-1, sorted=True)
    assert torch.equal(idx, ref['order'])
    ck, cs, ce = c['ckey'].double().t(), c['cshr'].double(), c['csel'].double().t()
    sim = get_similarity(ck, cs, ck[:, idx], ce[:, idx])                      # [n, P]
    scale = max(1.0, float(B.consol_aff_true(c['ckey'], c['cshr'], c['ckey'][idx], c['csel'][idx])['mag'].max()))
    assert float((sim.t() - ref['S']).abs().max()) <= 1e-12 * scale
    aff, _ = topk_softmax(sim, None)
    assert float((aff.t() - ref['w']).abs().max()) <= 1e-9
    for o, v in enumerate(vals):
        assert float((v.double().t() @ aff - ref['y'][o].t()).abs().max()) <= 1e-9
    assert float(((cs[None, :] @ aff)[0] - ref['shr']).abs().max()) <= 1e-9


def test_summarize_ref_is_the_reference_arithmetic_in_float64():
    K, HW, C, Q = 3, 129, 64, 16
    feat, wl, m = B.make_summarize(3, 'plain', K, HW, C)
    ref = B.summarize_ref(feat, wl, m, HW)
    m5 = m.double()[None, :, :, None, None].reshape(1, K, HW, 1, 1)
    rep = torch.cat([m5.expand(-1, -1, -1, -1, Q // 2), (1 - m5).expand(-1, -1, -1, -1, Q // 2)], -1)
    weights = wl.double().view(1, K, HW, 1, Q).sigmoid() * rep                # object_summarizer: [b, k, h, w, q] with (h, w) = (HW, 1)
    sums = torch.einsum('bkhwq,bkhwc->bkqc', weights, feat.double().view(1, K, HW, 1, C))
    area = weights.flatten(2, 3).sum(2).unsqueeze(-1)
    assert float((torch.cat([sums, area], -1)[0] - ref['y']).abs().max()) <= 1e-12 * HW


def test_fixed_point_conversion_reference():
    """fx_to_f32 against what can be checked independently: exact below 2^24 units of the last place, and the two double-rounding cases."""
    assert B.fx_to_f32(2 ** 40) == 1.0 and B.fx_to_f32(2 ** 64 - 1) == np.float32(2.0 ** 24) and B.fx_to_f32(1) == np.float32(2.0 ** -40)
    assert B.fx_to_f32(2 ** 53 + 2 ** 29 + 1) == np.nextafter(np.float32(8192), np.float32(1e9))      # above the tie: up
    assert B.fx_to_f32(2 ** 53 + 2 ** 29) == np.float32(8192)                                         # the tie: to even
    assert B.fx_to_f32(2 ** 53 + 3 * 2 ** 29) == np.float32(8192) + np.float32(2.0 ** -9)             # the tie above an odd significand: up
    for d in B.fx_values(0, 200):
        if d < 2 ** 53:
            assert B.fx_to_f32(d) == np.float32(float(d) * 2.0 ** -40)


# ---- the interpreter passes every case of the shared list -------------------------------------------------------------------------------
@pytest.mark.parametrize('n,k,kind,nzero', B.RANK_CASES)
def test_interpreter_rank_select_gather(n, k, kind, nzero):
    B.run_rank_case('cpu', mock, n, k, kind, nzero)


@pytest.mark.parametrize('n,P,regime', B.AFF_CASES)
def test_interpreter_consol_aff(n, P, regime):
    B.run_aff_case('cpu', mock, n, P, regime)


@pytest.mark.parametrize('n,P,C,K,skind,vkind,adjacent', B.READ_CASES)
def test_interpreter_consol_read(n, P, C, K, skind, vkind, adjacent):
    B.run_read_case('cpu', mock, n, P, C, K, skind, vkind, adjacent)


@pytest.mark.parametrize('n,P,K,regime,seed,keep', B.CHAIN_CASES)
def test_interpreter_chain(n, P, K, regime, seed, keep):
    B.run_chain_case('cpu', mock, n, P, K, regime, seed, keep)


@pytest.mark.parametrize('case', B.TICK_CASES)
def test_interpreter_usage_tick(case):
    B.run_tick_case('cpu', mock, *case)


@pytest.mark.parametrize('words', B.BW_LAUNCHES)
def test_interpreter_bank_write(words):
    B.run_bank_write_case('cpu', mock, words)


@pytest.mark.parametrize('n', [1, 255, 256, 257, 1000])
def test_interpreter_copy_fill_cast_axpy(n):
    B.run_misc_case('cpu', mock, n)


@pytest.mark.parametrize('K,HW,C,regime,f32_form', B.SUM_CASES)
def test_interpreter_summarize(K, HW, C, regime, f32_form):
    B.run_summarize_case('cpu', mock, K, HW, C, regime, f32_form)


@pytest.mark.parametrize('Bn,n8', [(1, 1), (3, 1), (1, 300), (3, 333)])
def test_interpreter_add_pe(Bn, n8):
    B.run_add_pe_case('cpu', mock, Bn, n8)


def test_the_case_lists_reach_every_size():
    assert {c[0] for c in B.RANK_CASES} >= {1, 2, 17, 255, 256, 257, 1000, 4100, 8100} and {c[2] for c in B.RANK_CASES} == set(B.USAGE_KINDS)
    assert any(c[1] == 1 for c in B.RANK_CASES) and any(c[1] == c[0] for c in B.RANK_CASES) and any(c[1] == 128 for c in B.RANK_CASES)
    assert (1000, 30) in {(c[0], c[3]) for c in B.RANK_CASES} and (1, 300) in {(c[0], c[3]) for c in B.RANK_CASES}
    assert {c[0] for c in B.AFF_CASES} >= {1, 31, 32, 33, 270, 1000} and {c[1] for c in B.AFF_CASES} >= {1, 15, 16, 17, 65, 128, 136}
    assert {c[2] for c in B.AFF_CASES} == set(B.AFF_REGIMES)
    assert {c[0] for c in B.READ_CASES} >= {1, 32, 33, 255, 256, 257, 513, 1000, 8100} and {c[1] for c in B.READ_CASES} >= {1, 16, 17, 128, 129, 136}
    assert {c[2] for c in B.READ_CASES} == {128, 256, 384} and {c[3] for c in B.READ_CASES} >= {1, 2, 5} and {c[6] for c in B.READ_CASES} == {True, False}
    assert {c[4] for c in B.READ_CASES} >= {'onehot', 'ramp', 'flat', 'far', 'video3', 'video8'} and {c[5] for c in B.READ_CASES} == set(B.VALUE_KINDS)
    assert {w for l in B.BW_LAUNCHES for w in l} >= set(B.BW_WORDS)
    assert {c[1] for c in B.SUM_CASES} >= {1, 4, 127, 128, 129, 1025, 1620} and {c[3] for c in B.SUM_CASES} == set(B.SUM_REGIMES)
    assert {c[0] for c in B.SUM_CASES} == {1, 3} and {c[2] for c in B.SUM_CASES} == {64, 256} and {c[4] for c in B.SUM_CASES} == {True, False}
    assert {c[5] for c in B.TICK_CASES} == {None, 'A', 'B', 'U'}


# ---- the checks bite: float64 restatements with one fault each ----------------------------------------------------------------------------
def restate_aff(c, pk, pe, idx, n, P, fault=None):
    """CONSOL_AFF in float64, stored as the launch stores it: S f32 [P + 2, ldS] between sentinel rows, colmax keys."""
    ck, cs, ce, pk, pe = c['ckey'].double(), c['cshr'].double(), c['csel'].double(), pk.double(), pe.double()
    sc = (cs[idx % n][:, None] if fault == 'proto_shr' else cs[None]) * (1.0 if fault == 'no_0125' else 0.125)
    S = torch.empty((P, n), dtype=F64)
    for p in range(P):
        e = ce if fault == 'cand_sel' else pe[p][None]
        if fault == 'no_bsq':
            S[p] = -(e * ck * ck - 2 * e * ck * pk[p][None]).sum(1)
        else:
            S[p] = -(e * (ck - pk[p][None]) ** 2).sum(1)
    S = S * sc
    ldS = O.OpList.consol_lds(n)
    out = torch.full((P + 2, ldS), B.SENT_F)
    out[:P] = 0.0 if fault == 'pad0' else B.NEG_INF
    out[:P, :n] = S.float()
    cm = torch.full((P + 3,), B.SENT_I, dtype=I32)
    cm[:P] = torch.from_numpy(B.f2key(out[:P, :n].max(1).values).view(np.int32).copy())
    return out, cm


AFF_FAULTS = ['no_0125', 'cand_sel', 'proto_shr', 'no_bsq', 'pad0']
AFF_MUT_CASES = [c for c in B.AFF_CASES if c[0] <= 270]


def _aff_outcome(fault):
    failed = 0
    for n, P, regime in AFF_MUT_CASES:
        c = B.make_consol(1000 * n + P, regime, n, P)
        pk, pe, idx = B.pick_prototypes(c, P)
        S, cm = restate_aff(c, pk, pe, idx, n, P, fault)
        try:
            B.check_consol_aff(S, cm, B.consol_aff_true(c['ckey'], c['cshr'], pk, pe), n, P)
        except AssertionError:
            failed += 1
    return failed


def test_consol_aff_restatement_passes_and_every_fault_fails():
    assert _aff_outcome(None) == 0
    for f in AFF_FAULTS:
        assert _aff_outcome(f) > 0, f


def restate_read(S, colmax, before, cshr, n, P, src, dst, fault=None):
    """CONSOL_READ from the S / colmax given: the weights as fp32 exponentials of the fp32 difference (an overflow or a column of zeros
    shows as it would in the kernel), everything behind them in float64.  Returns (banks, out_shr [P + 2])."""
    K = len(before)
    keys = B.keys_of(colmax)[:P]
    if fault == 'colmax_next':
        keys = np.roll(keys, -1)
    m = B.key2f(keys).numpy()
    with np.errstate(all='ignore'):
        w32 = np.exp((B.cpu(S)[:P, :n].numpy() - m[:, None]).astype(np.float32)).astype(np.float32)
    w = torch.from_numpy(w32.astype(np.float64))
    wnum = w.clone()
    if fault == 'drop_lo':
        wnum = torch.from_numpy(w32).to(BF16).double()
    z = w.sum(1)
    if fault == 'dup_last':
        wnum[:, n - 1] *= 2
        z = z + w[:, n - 1]
    if fault == 'skip_chunk_z':
        z = z - w[:, :256].sum(1) * (1.0 if n > 256 else 0.5)
    cs = cshr.double()
    with np.errstate(all='ignore'):
        shr = (w @ cs) / (float(n) if fault == 'shr_by_n' else z)
    banks = [b.clone() for b in before]
    order = list(range(K))
    if fault == 'swap_objects':
        order = order[1:] + order[:1]
    s0 = src + 1 if fault == 'src_plus1' else src
    d0 = dst + 1 if fault == 'dst_plus1' else dst
    for o in range(K):
        y = (wnum @ before[order[o]][s0:s0 + n].double()) / z[:, None]
        banks[o][d0:d0 + P] = y.to(BF16)
    out_shr = torch.full((P + 2,), B.SENT_F)
    out_shr[:P] = shr.float()
    return banks, out_shr


READ_FAULTS = ['dup_last', 'colmax_next', 'skip_chunk_z', 'src_plus1', 'dst_plus1', 'swap_objects', 'shr_by_n']
READ_MUT_CASES = [c for c in B.READ_CASES if c[0] <= 1000]


def _read_operands(n, P, C, K, skind, vkind, adjacent):
    """The S / colmax a CONSOL_READ case reads (hand-built, or the float64 restatement of CONSOL_AFF) and its banks."""
    seed = 7 * n + P + C + K
    ldS = O.OpList.consol_lds(n)
    if skind in ('onehot', 'ramp'):
        S, cm = B.hand_S(skind, n, P, ldS)
        cshr = torch.rand((n,), generator=torch.Generator().manual_seed(seed)) * 9 + 1
    else:
        c = B.make_consol(seed, skind, n, P)
        pk, pe, idx = B.pick_prototypes(c, P)
        S, cm = restate_aff(c, pk, pe, idx, n, P)
        cshr = c['cshr']
    rc = B.ReadCase('cpu', B.Bufs('cpu'), n, P, C, K, vkind, adjacent, seed)
    return S, cm, cshr, rc, ldS


def _read_outcome(fault, cases=READ_MUT_CASES):
    failed, worst = 0, 0.0
    for case in cases:
        n, P, C, K = case[:4]
        S, cm, cshr, rc, ldS = _read_operands(*case)
        banks, out_shr = restate_read(S, cm, rc.before, cshr, n, P, rc.src, rc.dst, fault)
        ref = B.consol_read_ref(S, cm, rc.before, cshr, n, P, rc.src, ldS)
        try:
            ry, rs = B.check_consol_read(banks, rc.before, out_shr, ref, P, rc.dst)
            worst = max(worst, ry)
        except AssertionError:
            failed += 1
    return failed, worst


def test_consol_read_restatement_passes_and_every_fault_fails():
    assert _read_outcome(None)[0] == 0
    for f in READ_FAULTS:
        assert _read_outcome(f)[0] > 0, f


def test_a_dropped_lo_term_of_the_weight_split():
    """hi alone keeps 8 bits of every weight: the numerator moves by up to ub sum w |V| / z, the size of the bf16 store's own half ulp.  The y
    bound is ub |y| for that store plus about 1e-5 of the magnitude sum, so it has no room for a second ub-sized term: wherever the store's
    rounding lands near a tie, the shifted value rounds the other way and leaves the bound.  Measured over the shared list (n <= 1000): the
    fault FAILS 6 of 13 cases -- video3 / x64, video8 / sparse, far / sparse, video3 / randn and both ramps -- and is invisible, with the ratio
    unchanged, exactly where nothing is dropped: one-hot columns and `flat` (weights 0 and 1 are bf16 numbers; ratio 0.794 there is the store's
    own rounding) and the columns that one weight of 1 dominates (constant values under video8 / sparse_sel: ratio 1e-13).  So the split is
    NOT behind the bf16 store: the check sees it, and it is listed with the faults that bite."""
    failed, worst = _read_outcome('drop_lo')
    print(f'bank_ref64 drop_lo: fails {failed} of {len(READ_MUT_CASES)} cases; worst ratio on the cases it passes {worst:.3g}')
    assert failed >= 3 and worst <= 1.0
    flat = [c for c in READ_MUT_CASES if c[4] in ('flat', 'onehot')]
    assert _read_outcome('drop_lo', flat)[0] == 0


def restate_rank(use, life, n, k, fault=None):
    with np.errstate(all='ignore'):
        q = use.numpy().astype(np.float32) / life.numpy().astype(np.float32)
    if fault == 'use_only':
        q = use.numpy().astype(np.float32)
    i = np.arange(n)
    above = q[None, :] > q[:, None]
    eq = q[None, :] == q[:, None]
    if fault == 'ascending':
        above = q[None, :] < q[:, None]
    tie = (i[None, :] > i[:, None]) if fault == 'tie_reversed' else (i[None, :] < i[:, None])
    if fault == 'ge':
        tie = i[None, :] != i[:, None]
    rank = (above | (eq & tie)).sum(1)
    order = np.full((k + 5,), B.SENT_I, dtype=np.int64)
    for t in range(n):
        if rank[t] < k:
            order[rank[t]] = t
    return torch.from_numpy(order)


RANK_FAULTS = ['use_only', 'ascending', 'tie_reversed', 'ge', 'prev_order']
RANK_MUT_CASES = [c for c in B.RANK_CASES if c[0] <= 1000]


def _rank_outcome(fault):
    failed = 0
    for n, k, kind, nzero in RANK_MUT_CASES:
        use, life = B.make_usage(n + k, kind, n)
        g = torch.Generator().manual_seed(n)
        srcs = [torch.randint(-2 ** 31, 2 ** 31 - 1, (n, w), generator=g, dtype=torch.int64).to(I32) for w in (4, 64)]
        order = restate_rank(use, life, n, k, None if fault == 'prev_order' else fault)
        through = restate_rank(life, use + 1, n, k)[:k] if fault == 'prev_order' else order[:k]          # (the order an earlier call left)
        side = []
        for s in srcs:
            d = torch.full((k + 2, s.shape[1]), B.SENT_I, dtype=I32)
            ok = through != B.SENT_I
            d[:k][ok] = s[through[ok]]
            side.append(d)
        cleared = torch.full((nzero + 7,), B.SENT_I, dtype=I32)
        cleared[:nzero] = 0
        try:
            B.check_rank(dict(order=order, side=side, cleared=cleared), dict(use=use, life=life, srcs=srcs, nzero=nzero), n, k)
        except AssertionError:
            failed += 1
    return failed


def test_rank_restatement_passes_and_every_fault_fails():
    assert _rank_outcome(None) == 0
    for f in RANK_FAULTS:
        assert _rank_outcome(f) > 0, f


def test_fixed_point_delta_through_a_double_fails_from_2_pow_53_only():
    vals = B.fx_values(3, 400)
    wrong = [d for d in vals if np.float32(float(d) * 2.0 ** -40) != B.fx_to_f32(d)]
    assert wrong and all(d >= 2 ** 53 for d in wrong) and {2 ** 53 + 2 ** 29 + 1, 2 ** 63 + 2 ** 39 + 1} <= set(wrong)
    use = torch.zeros(len(vals))
    via_double = torch.from_numpy(np.array([np.float32(float(d) * 2.0 ** -40) for d in vals], dtype=np.float32))
    assert not B.same_bits(via_double, B.tick_use_ref(use, B.u64_tensor(vals), len(vals), True))
    small = [d for d in vals if d < 2 ** 53]
    assert B.same_bits(torch.from_numpy(np.array([np.float32(float(d) * 2.0 ** -40) for d in small], dtype=np.float32)),
                       B.tick_use_ref(torch.zeros(len(small)), B.u64_tensor(small), len(small), True))


def restate_summarize(feat, wl, m, fault=None):
    f, wl, m = feat.double(), wl.double(), m.double()[..., None]
    Q = wl.shape[-1]
    a, b = (1 - m, m) if fault == 'one_minus_first' else (m, 1 - m)
    w = torch.sigmoid(wl) * torch.cat([a.expand(-1, -1, Q // 2), b.expand(-1, -1, Q // 2)], -1)
    area = w.sum(1)
    if fault == 'area_wrong_half':
        area = torch.cat([area[:, Q // 2:], area[:, :Q // 2]], 1)
    return torch.cat([torch.einsum('kpq,kpc->kqc', w, f), area[..., None]], -1).float()


def _sum_outcome(fault):
    failed = 0
    for K, HW, C, regime, f32_form in B.SUM_CASES:
        feat, wl, m = B.make_summarize(HW + C + K, regime, K, HW, C)
        stored = feat if f32_form else feat.to(BF16)
        try:
            B.check_summarize(restate_summarize(stored, wl, m, fault), B.summarize_ref(stored, wl, m, HW))
        except AssertionError:
            failed += 1
    return failed


def test_summarize_restatement_passes_and_every_fault_fails():
    assert _sum_outcome(None) == 0
    for f in ('one_minus_first', 'area_wrong_half'):
        assert _sum_outcome(f) > 0, f


def test_a_fill_one_word_long_fails():
    """The interpreter's outputs with one more word filled: the sentinel behind the fill gives it away."""
    def long_fill(ol, b):
        mock(ol, b)
        v = b['fill0']
        v[v.numel() - 3] = v[0]
    B.run_bank_write_case('cpu', mock, B.BW_LAUNCHES[0])
    with pytest.raises(AssertionError):
        B.run_bank_write_case('cpu', long_fill, B.BW_LAUNCHES[0])
