"""Float64 references of the pixel-memory read-out (csrc/affinity.hip: KEY_PREP, AFF_SCORE pass 0 / 1, AFF_SELECT, AFF_READOUT) with
per-element error bounds, the checks built on them, and the launch builders shared by tests/test_aff_ref64_cpu.py (the interpreter on the
host) and tests/test_gpu_aff_ref64.py (the HIP kernels).  TEST INFRASTRUCTURE ONLY.

Independent of tests/mock_exec.py and of the kernels: every reference reads the buffers a launch reads and applies the formulas of
include/cutie_hip.h and of the header of affinity.hip in float64.  No bound below is fitted to what a kernel returns; each follows from the
arithmetic, with u = 2^-24 (ref64.U32, fp32 round to nearest), ub = 2^-8 (ref64.U_BF16, bf16 round to nearest: 8 significant bits),
gamma_n = n u / (1 - n u) (+ n 2^-53 for the float64 sum itself; Higham, Accuracy and Stability, Lemma 3.1) and FTZ = 2^-126 per rounding
step for flushed denormals.

KEY_PREP (``key_prep_ref``).  v = [k^2 | k] (memory) or [-e | 2 k e] (query).  k and -e are fp32 values already; k*k and (2k)*e take ONE
fp32 rounding (2k is exact): v32 = v (1 + d), |d| <= u.  hi = bf16(v32), so |v32 - hi| <= ub |v32| and the difference is an fp32 number
(the error of a rounding to fewer bits is representable); lo = bf16(v32 - hi) loses at most ub of that: |hi + lo - v32| <= ub^2 |v32|.
Together |hi + lo - v| <= (u r + ub^2 (1 + u)) |v| + 4 FTZ =: the operand bound (r = 1 where a product was rounded, else 0), about
2^-16 |v|.  Where |v32| >= 2^-100 (or v32 == 0) no step can touch a denormal and the bits are decidable: hi == bf16(v32) and
lo == bf16(v32 - hi) exactly, v32 evaluated in fp32 in the kernel's order.  scale = shrinkage * 0.125 is exact.  c_j = sum_i e_i k_i^2:
64 terms of two roundings each, (e k) k, and 63 additions in some order: |c - c64| <= gamma_66 sum |e k^2| + 66 FTZ.

AFF_SCORE (``score_ref``).  From the STORED operands, A = Ahi + Alo, B = Bhi + Blo (exact in float64):
S_op = scale (A . B - c).  The kernel sums the 3 x 128 products hi*hi, hi*lo, lo*hi -- each exact in fp32, a product of two 8-bit
significands -- and -c in fp32 in some order (MFMA accumulation; the bound holds for any order): gamma_385 of the magnitude sum; what it
never adds is |Alo| . |Blo|; the last step, fma(scale, acc, pad), is one rounding.  With
mag = scale ((|Ahi| + |Alo|) . (|Bhi| + |Blo|) + |c|):
    |S - S_op| <= scale |Alo| . |Blo| + (gamma_386 + 2 u) mag + 390 FTZ (1 + scale).
The bound is proportional to mag, never to |S|: S cancels to zero for a good match, mag does not.
``score_true`` is the same matrix from the raw fp32 keys, S_true = -scale sum_i e_i (km_i - kq_i)^2.  The stored operands differ from
the true ones by the KEY_PREP bound, eps = u + ub^2 (1 + u) per operand, |lo| <= ub (1 + ub)(1 + u) |v| =: L |v|, and c by gamma_66:
with AB = |A_t| . |B_t| = sum e km^2 + 2 sum |km kq e|, ct = sum e kq^2 and mag_t = scale (AB + ct),
    |S - S_true| <= scale (((1 + eps)^2 - 1 + L^2) AB + gamma_66 ct) + (gamma_386 + 2 u)(1 + eps)^2 mag_t + 390 FTZ (1 + scale),
about 6.9e-5 mag_t: the dropped lo*lo term and the two operand splits are 2^-16 each, the fp32 accumulation 386 x 2^-24.

Tile maxima (``tile_max_ref``): max over the VALID tokens of a 16-token tile is 1-Lipschitz in the sup norm: the bound of a maximum is
the largest element bound of its tile.  ``select_ref``: exact, on order-preserving integer keys; compared by value.
``candidates_ref``: a token with S_op >= tau + bound must be in the list whatever the kernel's rounding, one with S_op < tau - bound
must not; the rest is undecided.

AFF_READOUT (``readout_ref``), from a GIVEN candidate list.  Selection is exact (value descending, ties to the lower token index; a
duplicated (value, index) entry takes one rank and leaves the next one empty with weight 0, as the kernel documents).  Weights: d_i =
fl(v_i - v_0) (|d| u absolute, hence a relative |d| u of its exponential), expf (2 ulp: 4 u relative), the sum of <= 64 positive terms
(gamma_64 and the weighted mean of the terms' own errors), one division: e_i' = e_i (1 + a_i), a_i = (|d_i| + 4) u, sum' = sum (1 + b),
|b| <= sum e a / sum e + gamma_64, so |w' - w| <= w ((1 + a_i)(1 + u) / (1 - b) - 1) + FTZ.  y = sum w V: <= 64 products and additions,
two roundings a term: gamma_128 sum |w V| + sum wb |V|, then the bf16 store, ub (|y| + that).  Usage, f32 atomics: a token's counter
takes m additions in arrival order: gamma_m sum w + sum wb.  Fixed point (2^-40): trunc(w32 2^40) is exact given w32 up to the
truncation, and integer sums are exact: sum (wb + 2^-40).

``pipeline_ref``: the chain from the raw keys.  With E_i the S_true bound of token i and Em the largest E among a query's selected
tokens, the kernel's logits are s_i + t_i, |t_i| <= E_i, so each weight moves by a factor within e^(+-(E_i + Em)):
|w' - w| <= w (e^(E_i + Em) - 1), to which the fp32 softmax bound above is added (on w e^(E_i + Em)).  A query is AMBIGUOUS when the
gap between its k-th and (k+1)-th true scores does not exceed the sum of their two bounds: its selected set is not fixed, it is left out
of the y comparison, and every token whose score reaches within the bounds of the k-th gets its largest possible weight,
min(1, e^(s_i + E_i - (s_0 - E_0))), added to its usage bound instead.  A case may leave out at most AMBIG_CAP of its queries
(test_aff_ref64_cpu.py asserts that for every seed in use, from the reference alone)."""
import torch

from ref64 import FTZ, U32, U64, U_BF16, check_bound           # noqa: F401  (check_bound: re-exported for the tests)

F64, F32, BF16, I32 = torch.float64, torch.float32, torch.bfloat16, torch.int32
NEG_INF = float('-inf')
AFF_CSTRIDE, AFF_WCAP, RO_PRUNE, RO_MAXK = 32, 256, 64, 64
AMBIG_CAP = 0.05
N_ACC = 3 * 128 + 1
EPS_SPLIT = U32 + U_BF16 ** 2 * (1 + U32)
LO_REL = U_BF16 * (1 + U_BF16) * (1 + U32)
FX = 2.0 ** -40


def gamma(n):
    return n * U32 / (1 - n * U32) + n * U64


def slots_of(ranges):
    return torch.cat([torch.arange(s, s + n) for s, n in ranges if n > 0])


def tiles_of(ranges):
    """Tile number of every valid token (in slots_of order) and the number of tiles G."""
    t, g = [], 0
    for _, n in ranges:
        if n > 0:
            t.append(g + torch.arange(n) // 16)
            g += -(-n // 16)
    return torch.cat(t), g


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.int64)


# ---- KEY_PREP ---------------------------------------------------------------------------------------------------------------------------
def key_prep_ref(key, aux, query):
    """v64 [n, 128], its bound, the fp32 image v32 the kernel splits, the side value (scale | c) with its bound."""
    k = key.detach().cpu().float()
    k64 = k.double()
    n = k.shape[0]
    one, zero = torch.ones((n, 64), dtype=F64), torch.zeros((n, 64), dtype=F64)
    if query:
        e = aux.detach().cpu().float()
        e64 = e.double()
        v64, v32, r = torch.cat([-e64, 2 * k64 * e64], 1), torch.cat([-e, (2 * k) * e], 1), torch.cat([zero, one], 1)
        terms = e64 * k64 * k64
        side, sbound = terms.sum(1), gamma(66) * terms.abs().sum(1) + 66 * FTZ
    else:
        v64, v32, r = torch.cat([k64 * k64, k64], 1), torch.cat([k * k, k], 1), torch.cat([one, zero], 1)
        side = aux.detach().cpu().double() * 0.125
        sbound = torch.full_like(side, FTZ)
    vb = (U32 * r + U_BF16 ** 2 * (1 + U32)) * v64.abs() + 4 * FTZ
    return dict(v=v64, vbound=vb, v32=v32, side=side, sbound=sbound, decidable=(v32.abs() >= 2.0 ** -100) | (v32 == 0))


def check_key_prep(hi, lo, side, ref, what=''):
    hi, lo, side = hi.detach().cpu(), lo.detach().cpu(), side.detach().cpu()
    n = ref['v'].shape[0]
    r = check_bound(hi[:n].double() + lo[:n].double(), ref['v'], ref['vbound'], what=what + ' hi+lo')
    rs = check_bound(side[:n].double().view(-1, 1), ref['side'].view(-1, 1), ref['sbound'].view(-1, 1), what=what + ' side')
    v32, m = ref['v32'], ref['decidable']
    hw = v32.to(BF16)
    lw = (v32 - hw.float()).to(BF16)
    assert torch.equal(bits(hi[:n])[m], bits(hw)[m]), (what, 'hi != bf16(v32)', int((bits(hi[:n]) != bits(hw))[m].sum()))
    assert torch.equal(bits(lo[:n])[m], bits(lw)[m]), (what, 'lo != bf16(v32 - hi)', int((bits(lo[:n]) != bits(lw))[m].sum()))
    return max(r, rs)


# ---- AFF_SCORE --------------------------------------------------------------------------------------------------------------------------
def score_ref(Ahi, Alo, scale, Bhi, Blo, cq, ranges, HW):
    """S_op [HW, N], its bound and the magnitude sum, from the stored operands (N = the valid tokens in slots_of order)."""
    sl = slots_of(ranges)
    ah, al, sc = Ahi.detach().cpu()[sl].double(), Alo.detach().cpu()[sl].double(), scale.detach().cpu()[sl].double()
    bh, bl, c = Bhi.detach().cpu()[:HW].double(), Blo.detach().cpu()[:HW].double(), cq.detach().cpu()[:HW].double()
    S = ((bh + bl) @ (ah + al).t() - c[:, None]) * sc[None]
    mag = ((bh.abs() + bl.abs()) @ (ah.abs() + al.abs()).t() + c.abs()[:, None]) * sc.abs()[None]
    bound = (bl.abs() @ al.abs().t()) * sc.abs()[None] + (gamma(N_ACC + 1) + 2 * U32) * mag + (N_ACC + 5) * FTZ * (1 + sc.abs()[None])
    return dict(S=S, bound=bound, mag=mag, slots=sl)


def score_true(mkey, mshr, qkey, qsel, ranges):
    """S_true [HW, N] from the raw fp32 keys, the kernel's bound against it and the magnitude sum."""
    sl = slots_of(ranges)
    km, sc = mkey.detach().cpu()[sl].double(), mshr.detach().cpu()[sl].double() * 0.125
    kq, e = qkey.detach().cpu().double(), qsel.detach().cpu().double()
    S = torch.empty((kq.shape[0], km.shape[0]), dtype=F64)
    for j0 in range(0, kq.shape[0], 16):
        d = km[None] - kq[j0:j0 + 16, None]
        S[j0:j0 + 16] = -(e[j0:j0 + 16, None] * d * d).sum(2) * sc[None]
    AB = e @ (km * km).t() + 2 * (kq * e).abs() @ km.abs().t()
    ct = (e * kq * kq).sum(1)[:, None]
    mag = (AB + ct) * sc[None]
    bound = sc[None] * (((1 + EPS_SPLIT) ** 2 - 1 + LO_REL ** 2) * AB + gamma(66) * ct) \
        + (gamma(N_ACC + 1) + 2 * U32) * (1 + EPS_SPLIT) ** 2 * mag + (N_ACC + 5) * FTZ * (1 + sc[None])
    return dict(S=S, bound=bound, mag=mag, slots=sl)


def tile_max_ref(S, bound, ranges):
    """[HW, G] maxima over the valid tokens of each 16-token tile, and the largest element bound of the tile."""
    ms, bs, o = [], [], 0
    HW = S.shape[0]
    for _, n in ranges:
        if n <= 0:
            continue
        T = -(-n // 16)
        s = torch.full((HW, T * 16), NEG_INF, dtype=F64)
        b = torch.zeros((HW, T * 16), dtype=F64)
        s[:, :n], b[:, :n] = S[:, o:o + n], bound[:, o:o + n]
        ms.append(s.view(HW, T, 16).max(2).values)
        bs.append(b.view(HW, T, 16).max(2).values)
        o += n
    return torch.cat(ms, 1), torch.cat(bs, 1)


# ---- AFF_SELECT -------------------------------------------------------------------------------------------------------------------------
def select_ref(gmax, k):
    """The k-th largest of every row of gmax [rows, G] (f32), exact; -inf when G < k.  NaN is out of scope."""
    g = gmax.detach().cpu().float().contiguous()
    if g.shape[1] < k:
        return torch.full((g.shape[0],), NEG_INF)
    i = g.view(I32)
    key = torch.where(i < 0, i ^ 0x7fffffff, i)                              # order-preserving: negative floats in reverse
    kth = torch.sort(key, dim=1, descending=True).values[:, k - 1].contiguous()
    return torch.where(kth < 0, kth ^ 0x7fffffff, kth).view(F32)


def candidates_ref(S, bound, tau):
    t = tau.detach().cpu().double()[:, None]
    return S >= t + bound, S < t - bound


def check_candidates(cv, ci, count, *, S, bound, tau, ranges, gmax, top_k, cap, sent_v, sent_i, what=''):
    """The candidate lists of pass 1 (cv / ci [HW, cap], count [HW]) as sets, against S_op: see the issue list in test_gpu_aff_ref64.py.
    Returns (worst |err| / bound, V [HW, N]: the stored value of every listed token, NaN elsewhere, for comparisons between forms)."""
    cv, ci, count, tau, gmax = cv.detach().cpu(), ci.detach().cpu(), count.detach().cpu(), tau.detach().cpu().float(), gmax.detach().cpu().float()
    HW, N = S.shape
    sl = slots_of(ranges)
    tile, G = tiles_of(ranges)
    lut = torch.full((int(sl.max()) + 1,), -1, dtype=torch.int64)
    lut[sl] = torch.arange(N)
    must, absent = candidates_ref(S, bound, tau)
    V = torch.full((HW, N), float('nan'), dtype=F32)
    worst = 0.0
    for j in range(HW):
        n = int(count[j])
        assert 0 <= n <= cap, (what, j, 'count', n)
        idx, val = ci[j, :n].long(), cv[j, :n]
        assert bool((cv[j, n:] == sent_v).all()) and bool((ci[j, n:] == sent_i).all()), (what, j, 'an entry past count was written')
        assert bool(((idx >= 0) & (idx < lut.numel())).all()), (what, j, 'token index outside the bank')
        col = lut[idx]
        assert bool((col >= 0).all()), (what, j, 'a token outside the ranges')
        assert torch.unique(col).numel() == n, (what, j, 'duplicate token')
        d = (val.double() - S[j, col]).abs()
        assert bool((d <= bound[j, col]).all()), (what, j, 'candidate value outside the bound', float((d / bound[j, col]).max()))
        worst = max(worst, float((d / bound[j, col]).max()) if n else 0.0)
        present = torch.zeros(N, dtype=torch.bool)
        present[col] = True
        assert bool(present[must[j]].all()), (what, j, 'a token clearly above tau is missing', int((must[j] & ~present).sum()))
        assert not bool(present[absent[j]].any()), (what, j, 'a token clearly below tau is listed')
        if G >= top_k:
            assert n >= min(top_k, N), (what, j, 'fewer than top_k candidates', n)
        tm = torch.full((G,), NEG_INF).scatter_reduce(0, tile[col], val, 'amax')
        hot = gmax[j, :G] >= tau[j]
        assert torch.equal(bits(tm[hot]), bits(gmax[j, :G][hot])), (what, j, 'the best candidate of a tile is not its pass-0 maximum, bit for bit',
                                                                     int((bits(tm[hot]) != bits(gmax[j, :G][hot])).sum()))
        assert bool((val >= tau[j]).all()), (what, j, 'a candidate below tau', float(tau[j]), float(val.min()), int((val < tau[j]).sum()))
        V[j, col] = val
    return worst, V


def same_where_both(Va, Vb):
    """Every token listed by two forms carries the same bits."""
    both = ~torch.isnan(Va) & ~torch.isnan(Vb)
    return torch.equal(bits(Va)[both], bits(Vb)[both])


# ---- AFF_READOUT ------------------------------------------------------------------------------------------------------------------------
def rank_select(val, idx, top_k):
    """Exact selection from a list: (values [nsel], indices [nsel], assigned [nsel]); value descending, ties -> lower token index; a duplicated
    (value, index) pair takes one rank, the rank behind it stays unassigned (-inf, weight 0)."""
    n = val.numel()
    nsel = min(n, top_k)
    v, i = val.double(), idx.long()
    rank = (v[None] > v[:, None]).sum(1) + ((v[None] == v[:, None]) & (i[None] < i[:, None])).sum(1)
    sv, si, ok = torch.full((nsel,), NEG_INF, dtype=F64), torch.zeros((nsel,), dtype=torch.int64), torch.zeros((nsel,), dtype=torch.bool)
    m = rank < nsel
    sv[rank[m]], si[rank[m]], ok[rank[m]] = v[m], i[m], True
    return sv, si, ok


def softmax_ref(sv, extra=None):
    """float64 weights of the selected values (sv[0] is the largest) and the bound of their fp32 evaluation; extra: a relative change of
    every weight, (e^(E_i + Em) - 1), that the logits' own error adds (pipeline_ref)."""
    d = sv - sv[0]
    e = torch.where(sv > NEG_INF, torch.exp(d), torch.zeros_like(d))
    w = e / e.sum()
    a = (d.abs().nan_to_num(posinf=0.0) + 4) * U32
    b = float((e * a).sum() / e.sum()) + gamma(64)
    rel = (1 + a) * (1 + U32) / (1 - b) - 1
    if extra is not None:
        rel = (1 + extra) * (1 + rel) - 1
    return w, w * rel + FTZ


def readout_ref(cand_val, cand_idx, count, values, top_k, cap, nslots):
    """From the lists as given: y [K, HW, CV] with its bound, the usage column sums with the bounds of the f32-atomics and the fixed-point form."""
    cv, ci, cnt = cand_val.detach().cpu(), cand_idx.detach().cpu(), count.detach().cpu()
    HW = cnt.numel()
    Vs = [v.detach().cpu() for v in values]
    K, CV = len(Vs), Vs[0].shape[1]
    y, yb = torch.zeros((K, HW, CV), dtype=F64), torch.zeros((K, HW, CV), dtype=F64)
    use, ub_sum, use_n = torch.zeros(nslots, dtype=F64), torch.zeros(nslots, dtype=F64), torch.zeros(nslots, dtype=F64)
    for j in range(HW):
        n = min(int(cnt[j]), cap)
        if n == 0:
            continue
        sv, si, ok = rank_select(cv[j, :n], ci[j, :n], top_k)
        si = torch.where(ok, si, si[0])
        w, wb = softmax_ref(sv)
        for o in range(K):
            rows = Vs[o][si].double()
            y[o, j] = (w[:, None] * rows).sum(0)
            e = gamma(2 * RO_MAXK) * (w[:, None] * rows.abs()).sum(0) + (wb[:, None] * rows.abs()).sum(0) + 2 * RO_MAXK * FTZ
            yb[o, j] = e + U_BF16 * (y[o, j].abs() + e)
        use.index_add_(0, si, w)
        ub_sum.index_add_(0, si, wb)
        use_n.index_add_(0, si, torch.ones_like(w))
    yb = yb + FTZ                                                             # (an empty list: y == 0 with a bound that is not 0 / 0)
    return dict(y=y, ybound=yb, usage=use, ubound_f32=(use_n + 1) * U32 / (1 - (use_n + 1) * U32) * use + ub_sum + FTZ, ubound_fx=ub_sum + use_n * FX)


# ---- the whole chain from the raw keys ----------------------------------------------------------------------------------------------
def pipeline_ref(mkey, mshr, qkey, qsel, ranges, values, top_k, nslots):
    t = score_true(mkey, mshr, qkey, qsel, ranges)
    S, E, sl = t['S'], t['bound'], t['slots']
    HW, N = S.shape
    k = min(top_k, N)
    Vs = [v.detach().cpu() for v in values]
    K, CV = len(Vs), Vs[0].shape[1]
    y, yb = torch.zeros((K, HW, CV), dtype=F64), torch.zeros((K, HW, CV), dtype=F64)
    use, ub = torch.zeros(nslots, dtype=F64), torch.zeros(nslots, dtype=F64)
    ambiguous = torch.zeros(HW, dtype=torch.bool)
    W = torch.zeros((HW, N), dtype=F64)
    tops = torch.zeros((HW, k), dtype=torch.int64)
    for j in range(HW):
        order = torch.argsort(S[j], descending=True, stable=True)
        top = tops[j] = order[:k]
        sv, Ej = S[j, top], E[j, top]
        w, _ = softmax_ref(sv)
        W[j, top] = w
        use.index_add_(0, sl[top], w)
        if N > k and float(S[j, order[k - 1]] - S[j, order[k]]) <= float(E[j, order[k - 1]] + E[j, order[k]]):
            ambiguous[j] = True
            near = S[j] + E[j] >= S[j, order[k - 1]] - E[j, order[k - 1]]                # everything that can reach the k-th place, the top k included
            near[top] = True
            wmax = torch.exp((S[j] + E[j] - (S[j, order[0]] - E[j, order[0]])).clamp(max=0))
            ub.index_add_(0, sl[near], wmax[near] + FX)
            continue
        _, wb = softmax_ref(sv, extra=torch.expm1(Ej + Ej.max()))
        ub.index_add_(0, sl[top], wb + FX)
        for o in range(K):
            rows = Vs[o][sl[top]].double()
            y[o, j] = (w[:, None] * rows).sum(0)
            e = gamma(2 * RO_MAXK) * (w[:, None] * rows.abs()).sum(0) + (wb[:, None] * rows.abs()).sum(0) + 2 * RO_MAXK * FTZ
            yb[o, j] = e + U_BF16 * (y[o, j].abs() + e)
    return dict(S=S, E=E, mag=t['mag'], slots=sl, W=W, top=tops, y=y, ybound=yb, usage=use, ubound=ub, ambiguous=ambiguous)


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
REGIMES = ('randn0.8', 'video3', 'video8', 'sparse_sel', 'cluster', 'cluster_flat')


def make_keys(seed, regime, HW, ranges, nslots, frames=1):
    """mkey [nslots, 64], mshr [nslots], qkey / qsel [frames, HW, 64].  The slots outside the ranges hold key 0 with shrinkage 0: their score is
    scale x (..) = 0, above every real score (all <= 0) -- a kernel that takes one token too many of a ragged tile or of a range shows it as a
    tile maximum, as a candidate and, through the NaN value rows of those slots, in y.  'cluster' draws the shrinkage per token as
    test_gpu_kernels.py's _affinity_build(cluster=True) does; 'cluster_flat' gives every token the same, so that the 16 tokens of a run score within 1e-4."""
    g = torch.Generator().manual_seed(seed)
    sl = slots_of(ranges)
    N = sl.numel()
    rn = lambda *s: torch.randn(s, generator=g)
    qsel = torch.rand((frames, HW, 64), generator=g)
    shr = torch.rand((N,), generator=g) * 2 + 1
    if regime in ('video3', 'video8'):
        a = 3.0 if regime == 'video3' else 8.0
        qkey = rn(frames, HW, 64) * a
        copy = torch.arange(N) // HW                                         # memory = noisy copies of the (first) query frame, sigma 0.01 .. 1
        sigma = 10.0 ** (-2 + 2 * (copy.float() / max(1, int(copy.max()))))
        mk = qkey[0][torch.arange(N) % HW] + rn(N, 64) * sigma[:, None]
        shr = torch.rand((N,), generator=g) * 9 + 1
    elif regime in ('cluster', 'cluster_flat'):
        qkey = rn(frames, HW, 64) * 0.8
        mk = (rn(-(-N // 16), 64) * 0.8)[torch.arange(N) // 16] + rn(N, 64) * 1e-5
        if regime == 'cluster_flat':
            shr = torch.full((N,), 2.0)
    else:
        qkey, mk = rn(frames, HW, 64) * 0.8, rn(N, 64) * 0.8
        if regime == 'sparse_sel':
            qsel = (torch.rand((frames, HW, 64), generator=g) < 0.06).float()
            qsel[..., 0] = 1.0
    mkey = torch.zeros((nslots, 64))
    mshr = torch.zeros((nslots,))
    mkey[sl], mshr[sl] = mk, shr
    return mkey, mshr, qkey.contiguous(), qsel.contiguous()


# ---- buffers between guards, launch builders ------------------------------------------------------------------------------------------
PAD = 512
SENT_F, SENT_I = -1234.5, -12345


class Bufs:
    """Operands between NaN (integers: sentinel) elements, outputs between sentinel elements; `reset` restores the outputs."""

    def __init__(self, dev):
        self.dev, self.guards, self.outs, self.keep = dev, [], {}, []

    def operand(self, t):
        n = t.numel()
        buf = torch.full((n + 2 * PAD,), float('nan') if t.is_floating_point() else SENT_I, dtype=t.dtype)
        buf[PAD:PAD + n] = t.reshape(-1)
        buf = buf.to(self.dev)
        self.keep.append(buf)
        return buf[PAD:PAD + n].view(t.shape)

    def output(self, name, shape, dtype, fill=None):
        n = 1
        for s in shape:
            n *= s
        sent = SENT_F if dtype.is_floating_point else SENT_I
        buf = torch.full((n + 2 * PAD,), sent, dtype=dtype)
        if fill is not None:
            buf[PAD:PAD + n] = fill if not torch.is_tensor(fill) else fill.reshape(-1)
        buf = buf.to(self.dev)
        v = buf[PAD:PAD + n].view(shape)
        self.guards.append((buf, n, sent))
        self.outs[name] = (v, v.clone())
        return v

    def __getitem__(self, name):
        return self.outs[name][0]

    def guards_intact(self):
        return all(bool((b[:PAD] == s).all()) and bool((b[PAD + n:] == s).all()) for b, n, s in self.guards)

    def reset(self):
        for v, init in self.outs.values():
            v.copy_(init)

    def snapshot(self):
        return {n: v.clone() for n, (v, _) in self.outs.items()}


FORMS = {'nq1': dict(nq=1), 'nq2': dict(nq=2), 'nq2dma': dict(nq=2, dma=True), 'nq4': dict(nq=4)}


class AffCase:
    """One bank and `frames` query frames with every buffer of the read-out chain.  Query rows: HWp per frame (HW real ones, the operand
    rows behind them zero as in the product); `passes(tag, ...)` allocates the maxima / thresholds / lists of one pass pair."""

    def __init__(self, dev, *, HW, ranges, regime='randn0.8', seed=0, K=1, top_k=30, frames=1, CV=256, cap=1024, HWp=None, keys=None):
        self.dev, self.HW, self.ranges, self.K, self.top_k, self.F, self.CV, self.cap = dev, HW, [r for r in ranges if r[1] > 0], K, top_k, frames, CV, cap
        self.HWp = HWp or -(-HW // 64) * 64
        self.nslots = max(s + n for s, n in self.ranges) + 3
        self.N = sum(n for _, n in self.ranges)
        self.G = sum(-(-n // 16) for _, n in self.ranges)
        self.Gld = -(-self.G // 64) * 64
        self.mkey, self.mshr, self.qkey, self.qsel = keys or make_keys(seed, regime, HW, self.ranges, self.nslots, frames)
        b = self.b = Bufs(dev)
        self.d_mkey, self.d_mshr, self.d_qkey, self.d_qsel = b.operand(self.mkey), b.operand(self.mshr), b.operand(self.qkey), b.operand(self.qsel)
        rows = frames * self.HWp
        self.Ahi, self.Alo, self.scale = b.output('Ahi', (self.nslots, 128), BF16), b.output('Alo', (self.nslots, 128), BF16), b.output('scale', (self.nslots,), F32)
        self.Bhi, self.Blo, self.cq = b.output('Bhi', (rows, 128), BF16, 0.0), b.output('Blo', (rows, 128), BF16, 0.0), b.output('cq', (rows,), F32, 0.0)
        g = torch.Generator().manual_seed(seed + 1000)
        vals = [(torch.randn((self.nslots, CV), generator=g)).to(BF16) for _ in range(K)]
        gap = torch.ones(self.nslots, dtype=torch.bool)
        gap[slots_of(self.ranges)] = False
        for v in vals:
            v[gap] = float('nan')
        self.values = vals
        self.d_values = [b.operand(v) for v in vals]
        self.vptrs = b.operand(torch.tensor([v.data_ptr() for v in self.d_values], dtype=torch.int64))

    def prep(self, ol):
        ol.key_prep(self.d_mkey, self.d_mshr, self.Ahi, self.Alo, self.scale, n=self.nslots, query=False)
        for f in range(self.F):
            r0 = f * self.HWp
            ol.key_prep(self.d_qkey[f], self.d_qsel[f], self.Bhi[r0:r0 + self.HW], self.Blo[r0:r0 + self.HW], self.cq[r0:r0 + self.HW], n=self.HW, query=True)

    def passes(self, tag):
        """gmax [rows, Gld] with tau [rows] right behind it (one buffer), the lists and the counters of one pass pair."""
        b, rows = self.b, self.F * self.HWp
        gb = b.output('gbuf' + tag, (rows * self.Gld + rows,), F32)
        return dict(gbuf=gb, gmax=gb[:rows * self.Gld].view(rows, self.Gld), tau=gb[rows * self.Gld:],
                    cval=b.output('cval' + tag, (rows, self.cap), F32), cidx=b.output('cidx' + tag, (rows, self.cap), I32),
                    count=b.output('count' + tag, (rows * AFF_CSTRIDE,), I32))

    def common(self, form):
        c = dict(HW=self.HW, HWp=self.HWp, ranges=self.ranges, cap=self.cap, **FORMS[form])
        if self.F > 1:
            c['frames'] = self.F
        return c

    def score0(self, ol, p, form, **kw):
        return ol.aff_score(self.Ahi, self.Alo, self.scale, self.Bhi, self.Blo, self.cq, p['gmax'], None, None, None, mode=0, **self.common(form), **kw)

    def select(self, ol, p, **kw):
        ol.aff_select(p['gmax'], p['tau'], HW=self.HW, HWp=self.HWp, G=self.G, top_k=self.top_k, clear_count=p['count'], frames=self.F, **kw)

    def score1(self, ol, p, form, skip=True, **kw):
        return ol.aff_score(self.Ahi, self.Alo, self.scale, self.Bhi, self.Blo, self.cq, p['tau'], p['cval'], p['cidx'], p['count'], mode=1,
                            gmax_precedes_tau=skip, **self.common(form), **kw)

    def readout(self, ol, p, name, usage_fx=True):
        b, F_ = self.b, self.F
        y = b.output('y' + name, (F_, self.K, self.HW, self.CV), BF16, float('nan'))
        use = b.output('use' + name, (F_, self.nslots), torch.int64 if usage_fx else F32, 0)
        ovf = b.output('ovf' + name, (1,), I32, 0)
        kw = dict(frames=F_, HWp=self.HWp, usage_stride=self.nslots) if F_ > 1 else {}
        ol.aff_readout(p['cval'], p['cidx'], p['count'], self.vptrs, use, y, ovf, HW=self.HW, cap=self.cap, top_k=self.top_k, K=self.K, CV=self.CV,
                       usage_fx=usage_fx, **kw)
        return y, use, ovf

    def frame_rows(self, t, f=0):
        """The HW real rows of frame f of a per-query buffer indexed by the stacked row."""
        return t[f * self.HWp:f * self.HWp + self.HW]

    def counts(self, p, f=0):
        return p['count'].view(-1, AFF_CSTRIDE)[f * self.HWp:f * self.HWp + self.HW, 0]

    def score_ref(self, f=0):
        r0 = f * self.HWp
        return score_ref(self.Ahi, self.Alo, self.scale, self.Bhi[r0:], self.Blo[r0:], self.cq[r0:], self.ranges, self.HW)


def run(ex, ol):
    ex.run(ol.finalize())
    if torch.cuda.is_available():
        torch.cuda.synchronize()


# ---- the checks of a stage's outputs, shared by the host and the GPU tests ----------------------------------------------------------
def verify_score0(case, p, f=0, sref=None, pad_written=True):
    """gmax of frame f within tile_max_ref's bound of S_op.  Padding columns, from the code: every kernel form stores the maxima of a whole
    4-tile group with one 16-byte store and puts -inf where the group has no tile, so columns [G, 4 ceil(G / 4)) are -inf and the columns
    behind them, up to Gld, are never written (pad_written=False: the interpreter, which writes the G real columns only).  The rows
    [HW, HWp) ARE written (the block computes them from the zero operand rows); nothing reads them.  Returns the worst ratio."""
    sref = sref or case.score_ref(f)
    gm, gb = tile_max_ref(sref['S'], sref['bound'], case.ranges)
    got = case.frame_rows(p['gmax'], f).detach().cpu()
    G, G4 = case.G, -(-case.G // 4) * 4
    assert bool((got[:, G:G4] == (NEG_INF if pad_written else SENT_F)).all()), 'a padding tile of the last group is not -inf'
    assert bool((got[:, G4:] == SENT_F).all()), 'a column behind the last 4-tile group was written'
    return check_bound(got[:, :G], gm, gb, what='gmax')


def verify_select(case, p, f=0):
    got = case.frame_rows(p['tau'], f).detach().cpu()
    want = select_ref(case.frame_rows(p['gmax'], f)[:, :case.G], case.top_k)
    assert bool((got == want).all()), ('tau is not the exact top_k-th largest tile maximum', int((got != want).sum()))
    pad = p['tau'][f * case.HWp + case.HW:(f + 1) * case.HWp].detach().cpu()
    assert bool((pad == SENT_F).all()), 'the tau of a padding row was written'


def verify_score1(case, p, f=0, sref=None, what=''):
    sref = sref or case.score_ref(f)
    r0 = f * case.HWp
    cnt = p['count'].view(-1, AFF_CSTRIDE).detach().cpu()
    # (the selection launch clears the counters of the real queries of ONE frame, of every stacked row otherwise: select_side_jobs)
    assert bool((cnt[r0 + case.HW:r0 + case.HWp, 0] == (SENT_I if case.F == 1 else 0)).all()), 'a padding row has candidates'
    assert bool((cnt[:, 1:] == SENT_I).all()), 'a word between two counters was written'
    for n in ('cval', 'cidx'):
        pad = p[n][r0 + case.HW:r0 + case.HWp].detach().cpu()
        assert bool((pad == (SENT_F if n == 'cval' else SENT_I)).all()), 'the list of a padding row was written'
    return check_candidates(case.frame_rows(p['cval'], f), case.frame_rows(p['cidx'], f), cnt[r0:r0 + case.HW, 0], S=sref['S'], bound=sref['bound'],
                            tau=case.frame_rows(p['tau'], f), ranges=case.ranges, gmax=case.frame_rows(p['gmax'], f), top_k=case.top_k, cap=case.cap,
                            sent_v=SENT_F, sent_i=SENT_I, what=what)


def usage_float(use):
    """Fixed-point (int64 holding the unsigned 2^-40 counters) or f32 usage as float64."""
    u = use.detach().cpu()
    return u.double() * FX if u.dtype == torch.int64 else u.double()


def verify_readout(case, p, y, use, ovf, f=0, what=''):
    """y and usage of frame f within readout_ref's bounds of the lists as they are; ovf == 0."""
    r0 = f * case.HWp
    cnt = p['count'].view(-1, AFF_CSTRIDE)[r0:r0 + case.HW, 0]
    ref = readout_ref(case.frame_rows(p['cval'], f), case.frame_rows(p['cidx'], f), cnt, case.values, case.top_k, case.cap, case.nslots)
    yy = y[f].detach().cpu()
    ry = check_bound(yy.reshape(-1, case.CV), ref['y'].reshape(-1, case.CV), ref['ybound'].reshape(-1, case.CV), what=what + ' y')
    fx = use.dtype == torch.int64
    ru = check_bound(usage_float(use[f]).view(-1, 1), ref['usage'].view(-1, 1), (ref['ubound_fx'] if fx else ref['ubound_f32']).view(-1, 1) + FX * 1e-6,
                     what=what + ' usage')
    assert int(ovf) == 0, 'overflow counter'
    return ry, ru


# ---- the cases of the end-to-end chain (the seeds whose share of ambiguous queries test_aff_ref64_cpu.py holds under the cap) -------
CHAIN_HW, CHAIN_RANGES, CHAIN_NSLOTS = 129, [(3, 370), (400, 37), (512, 603)], 1118
CHAIN_CASES = [('randn0.8', 2), ('video3', 4), ('video8', 4), ('cluster', 7)]


# ---- hand-built candidate lists for AFF_READOUT alone ------------------------------------------------------------------------------
def hand_lists(top_k, cap, nslots, seed=0):
    """(cand_val [R, cap], cand_idx [R, cap], count [R], groups): one list per query row -- the counts around every path (0, 1, top_k - 1,
    top_k, RO_PRUNE, RO_PRUNE + 1, 128, 129, cap - 1, cap); ties exactly at the top_k-th value with and without the prune, the top_k-th value
    repeated 40 times, all values equal, a duplicated (value, index) entry, -inf inside a list, a ladder 0, -1, -2 .. (weights down to
    e^-40) -- and every tie list in reversed and in random order as well: `groups` lists the rows that hold the same list (same result,
    bit for bit)."""
    g = torch.Generator().manual_seed(seed)
    rows, groups = [], []

    def idx(n):
        return torch.randperm(nslots, generator=g)[:n].to(I32)

    for n in (0, 1, top_k - 1, top_k, RO_PRUNE, RO_PRUNE + 1, 128, 129, cap - 1, cap):
        rows.append((torch.randn(n, generator=g) * 3, idx(n)))

    def three_orders(v, i):
        p = torch.randperm(v.numel(), generator=g)
        groups.append([len(rows), len(rows) + 1, len(rows) + 2])
        rows.extend([(v, i), (v.flip(0), i.flip(0)), (v[p], i[p])])

    for n in (RO_PRUNE, 100, 300):                                         # ties at the top_k-th value: 40 equal values across the cut
        hi_n = max(0, top_k - 7)
        v = torch.cat([torch.rand(hi_n, generator=g) + 1.0, torch.full((min(40, n - hi_n),), 0.5), torch.rand(max(0, n - hi_n - 40), generator=g) - 1.0])
        three_orders(v[:n], idx(n))
    three_orders(torch.full((200,), -2.25), idx(200))                     # all equal: the lowest top_k token indices win
    three_orders(-torch.arange(41.0), idx(41))                            # the ladder
    for n in (50, 90):                                                     # a duplicated (value, index) entry among the best
        v, i = torch.randn(n, generator=g) * 2, idx(n)
        best = int(v.argmax())
        v[(best + 1) % n], i[(best + 1) % n] = v[best], i[best]
        three_orders(v, i)
    for n in (40, 150):                                                    # -inf inside a list (n = 40: some are selected, with weight 0)
        v = torch.randn(n, generator=g)
        v[torch.randperm(n, generator=g)[:n // 2 - 3]] = NEG_INF
        three_orders(v, idx(n))
    R = len(rows)
    cv, ci = torch.full((R, cap), SENT_F), torch.full((R, cap), SENT_I, dtype=I32)
    cnt = torch.zeros(R, dtype=I32)
    for r, (v, i) in enumerate(rows):
        cv[r, :v.numel()], ci[r, :v.numel()], cnt[r] = v, i, v.numel()
    return cv, ci, cnt, groups
