"""Float64 / exact-integer references of the kernels that WRITE the memory later frames read -- csrc/bank.hip (RANK_SELECT, GATHER_ROWS,
CONSOL_AFF, CONSOL_READ), the bookkeeping kernels of csrc/elementwise.hip (BANK_WRITE, USAGE_TICK, AXPY, COPY2D, MEMSET32, CAST), SUMMARIZE
and ADD_PE -- with per-element error bounds, the operand regimes, the shared case list and the launch builders used by
tests/test_bank_ref64_cpu.py (the interpreter on the host) and tests/test_gpu_bank_ref64.py (the HIP kernels).  TEST INFRASTRUCTURE ONLY.

Independent of tests/mock_exec.py and of the kernels: every reference reads the buffers ONE launch reads and applies the formulas of
include/cutie_hip.h and of oracle/inference.py::_consolidate / oracle.net.get_similarity / topk_softmax / object_summarizer in float64 (or
in exact integers / numpy float32 where the result is exact).  No bound is fitted to what a kernel returns.  u = 2^-24 per fp32 operation
(round to nearest; the build has -ffp-contract=off and no fast-math), ub = 2^-8 per bf16 store, gamma_n = n u / (1 - n u) (+ n 2^-53 for
the float64 sum itself) of the MAGNITUDE sum for a sum whose longest path from a term to the result crosses n roundings -- whatever the order,
expf 2 ulp = 4 u relative (as aff_ref64.py states), FTZ = 2^-126 absolute per step that may flush a denormal.  A bound of 0 marks an exact
output, compared by bits.  The count n behind every gamma, from the kernel's longest path:

RANK_SELECT / GATHER_ROWS (exact).  order = the stable descending sort of the fp32 quotient use / life (numpy float32: one correctly
rounded division, the kernel's), ties -- +0 and -0 compare equal -- to the lower index; independent of torch.topk.  Side gathers and
GATHER_ROWS: src[order] bit for bit.  Sentinels: order and destination rows past k, the cleared buffer past i4, destination words between
the row and its stride.  The partial-rank scratch is internal.  Quotients that are fp32 denormals are not reachable (usage is a sum of
2^-40 units, life at most the frame count) and are left out.

CONSOL_AFF (``consol_aff_true``).  S_true[p,i] = -(shr_i / 8) sum_c e_pc (kc_ic - kp_pc)^2 from the raw fp32 keys, the differences taken in
float64 (a prototype that IS a candidate has S_true = 0 exactly).  The kernel expands the square: acc = sum_c (-e_c) fl(kc^2) + sum_c kc fl(2 kp e)
over 128 MFMA k slots (consol_sim_kernel: 2 x 16 instructions of 4 slots), then fl(fl(fl(acc - bsq) shr) 0.125).  A term of acc crosses 1
rounding of its operand (kc^2, or (2 kp) e; 2 kp is exact), 1 of its product, at most 128 accumulations, the subtraction and the product with
shr (x 0.125 is exact): n = 132.  bsq = sum_c fl(fl(e kp) kp): 2 roundings, 15 additions in the lane, 2 across the four channel groups
(rows_sum), the subtraction, shr: n = 21.  With A = sum e kc^2 + 2 sum |e kc kp| and B = sum e kp^2:
    |S - S_true| <= (shr / 8) (gamma_132 A + gamma_21 B) + 140 FTZ (1 + shr / 8),
proportional to the magnitude sum, never to |S|.  Exact: the padding [n, ldS) is -inf; colmax[p] decodes (either branch of the
order-preserving key) to a float EQUAL to the maximum of the stored S[p, :n]; rows past P keep their sentinels.

CONSOL_READ (``consol_read_ref``), from the S and colmax it is given.  d_i = fl(s_i - m) is ONE fp32 subtraction and is reproduced
exactly (numpy float32); w_i = expf(d_i): |w' - w| <= 4 u w + FTZ.  Numerator: hi = bf16(w'), lo = bf16(w' - hi) (the difference is exact),
|hi + lo - w'| <= ub^2 w'; the bf16 x bf16 products are exact in fp32; a chunk accumulates 2 x 256 terms (consol_read_part_kernel: 8 steps of
two 32-slot MFMAs) and the chunk sums are added in chunk order (consol_read_comb_kernel): n_a = 2 min(ldS, 256) + nchunk, so
|N' - N| <= ((1 + 4u)(1 + ub^2)(1 + gamma_na) - 1) sum w |V| + FTZ sum |V|.  Denominator, over the UNSPLIT w': 8 additions a step in the lane
(<= 64 a chunk), 2 across the lane groups, nchunk: n_z = min(ldS, 256) / 4 + 2 + nchunk; all terms are positive, so z' = z (1 + zeta),
|zeta| <= (1 + 4u)(1 + gamma_nz) - 1.  Then 1 / z' (<= 1 ulp = 2 u), the product (u) and the bf16 store: with theta = (1 + 2u)(1 + u) - 1,
phi = (theta + zeta) / (1 - zeta), rel = rel_N (1 + phi) + phi:  e = rel sum w |V| / z + FTZ terms, bound = e + ub (|y| + e).
out_shr: the same path with fp32 shrinkages -- one more rounding a term (the product w' shr), one division (2 u), no bf16 store: the SHARP
output, reported separately.  Exact: every bank row outside [dst, dst + P) keeps its bits for every object (the rows at src + n and outside
both regions hold NaN: a candidate read one too far shows even under a zero weight); for a one-hot column (one candidate at the maximum, all
others >= 110 below it: expf gives 0) the prototype IS that candidate's stored row and out_shr its shrinkage, bit for bit.

The chain as MemoryManager._compress issues it (``chain_ref``): _consolidate in float64 from the raw keys, values, shrinkages,
selections and counters.  The ranking is exact, so no prototype is left out (the generator keeps the P-th and (P+1)-th quotients distinct,
asserted on the host).  The kernel's S differs from S_true by at most E (above): the normalised weight of candidate i moves by a factor
within [e^-E_i / D+, e^E_i / D-], D+- = sum_j w_j e^(+-E_j) (the denominator is a weighted mean of the e^t_j) -- as aff_ref64.pipeline_ref
argues with the cruder e^(E_i + E_max); the fp32 read-out bound is added on the moved weights.

USAGE_TICK.  life + 1: one fp32 addition, reproduced exactly (numpy float32; life = 2^24 stays).  f32 delta: one fp32 addition, exact.
Fixed-point delta: the correctly rounded fp32 of the exact rational d / 2^40 (fractions.Fraction, round half to even on the integer
significand), then one fp32 addition: exact; d is cleared or kept per flags&2.

BANK_WRITE, COPY2D, MEMSET32 by bits; CAST against torch.Tensor.to both ways (ties to even, +-0, +-inf, NaN-ness, bf16 denormals); AXPY as
fl(fl(a x) + y) in numpy float32 by bits.

SUMMARIZE (``summarize_ref``).  weight = fl(sigma(wl) mq), mq = m (q < 8) or fl(1 - m): expf (4 u), the addition (u), the division (2 u)
-- the error of e^-wl enters sigma with a factor e / (1 + e) <= 1 -- one rounding for 1 - m, one for the product:
rw = (1 + 7u)(1 + u)^2 - 1, + 2 FTZ absolute (e^-wl overflows or sigma falls below 2^-126 at |wl| >= 87: the true weight is < FTZ there).
Sums: a thread adds 32 products (1 rounding each) in a row, 3 additions join the four pixel slices, the final kernel adds the nchunk
partials in chunk order: n_s = 36 + nchunk of sum |w f| (the area column: the same without the product).  Where every weight of a half is
an exact zero (m exactly 0 or 1) the sums are exact zeros.  Both feature forms.

ADD_PE.  The float64 sum; u |y| for the fp32 addition, ub (|y| + u |y|) for the bf16 store behind it."""
import math
from fractions import Fraction

import numpy as np
import torch

from aff_ref64 import SENT_F, SENT_I, Bufs, bits, gamma, key_prep_ref, check_key_prep   # noqa: F401  (shared with the read-out tests)
from cutie_amd import ops as O
from ref64 import FTZ, U32, U_BF16, check_bound

F64, F32, BF16, I32, I64 = torch.float64, torch.float32, torch.bfloat16, torch.int32, torch.int64
NEG_INF = float('-inf')
LIFE_EPS_BITS = int(np.float32(1e-7).view(np.int32))
N_AFF_ACC, N_AFF_BSQ = 132, 21
REL_EXP = 4 * U32


def cpu(t):
    return t.detach().cpu()


def same_bits(a, b):
    return torch.equal(bits(cpu(a)), bits(cpu(b)))


def f2key(x):
    """The order-preserving u32 key of fp32 values (bank.hip bank_f2key), as a numpy array."""
    b = cpu(x).contiguous().numpy().view(np.uint32)
    return np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key2f(k):
    k = np.asarray(k).astype(np.uint32)
    b = np.where(k >> 31, k & np.uint32(0x7fffffff), ~k).astype(np.uint32)
    return torch.from_numpy(b.view(np.float32).copy())


def keys_of(colmax):
    return cpu(colmax).contiguous().numpy().view(np.uint32)


# ---- RANK_SELECT / GATHER_ROWS -------------------------------------------------------------------------------------------------------
USAGE_KINDS = ('random', 'equal', 'pairs', 'zeros', 'fresh', 'big')


def make_usage(seed, kind, n):
    g = torch.Generator().manual_seed(seed)
    use, life = torch.rand((n,), generator=g) * 3, torch.floor(torch.rand((n,), generator=g) * 40) + 1
    if kind == 'equal':
        use, life = torch.full((n,), 0.75), torch.full((n,), 3.0)
    elif kind == 'pairs':                                                     # equal quotients from different pairs: 1/2 and 2/4
        use = torch.where(torch.arange(n) % 2 == 0, torch.tensor(1.0), torch.tensor(2.0))
        life = use * 2
        use[::5], life[::5] = 3.0, 4.0
    elif kind == 'zeros':                                                     # +0 and -0 usage: one tie class
        use = torch.where(torch.arange(n) % 3 == 0, torch.tensor(-0.0), torch.tensor(0.0))
        use[1::4] = torch.rand((len(range(1, n, 4)),), generator=g)
    elif kind == 'fresh':                                                     # tokens never read: use 0, life 1e-7
        fresh = torch.rand((n,), generator=g) < 0.4
        use[fresh], life[fresh] = 0.0, 1e-7
    elif kind == 'big':                                                       # quotients of 1e9, with ties among them
        use, life = torch.floor(torch.rand((n,), generator=g) * 8) * 25 + 50, torch.full((n,), 1e-7)
    return use.float().contiguous(), life.float().contiguous()


def rank_ref(use, life, k):
    with np.errstate(all='ignore'):
        q = cpu(use).numpy().astype(np.float32) / cpu(life).numpy().astype(np.float32)
    assert q.dtype == np.float32 and not np.isnan(q).any()
    return torch.from_numpy(np.argsort(-q, kind='stable')[:k].astype(np.int64)), q


def distinct_at(q, k):
    s = np.sort(q)[::-1]
    return k >= len(s) or s[k - 1] != s[k]


def check_rank(out, ops, n, k):
    """out: order [k + pad], side (list of [k + pad, words]), cleared; ops: use, life, srcs, zero words, the buffers' initial states."""
    want, _ = rank_ref(ops['use'], ops['life'], k)
    order = cpu(out['order']).long()
    assert torch.equal(order[:k], want), ('order', int((order[:k] != want).sum()), order[:k][:8].tolist(), want[:8].tolist())
    assert bool((order[k:] == SENT_I).all()), 'an entry of order past k was written'
    for a, (src, got) in enumerate(zip(ops['srcs'], out['side'])):
        assert same_bits(cpu(got)[:k], cpu(src)[want]), f'side gather {a} != src[order]'
        assert bool((cpu(got)[k:] == SENT_I).all()), f'side gather {a}: a row past k was written'
    z, nz = cpu(out['cleared']), ops['nzero']
    assert bool((z[:nz] == 0).all()) and bool((z[nz:] == SENT_I).all()), 'the cleared buffer'


def check_gather(dst, src, order, k, roww):
    dst, want = cpu(dst), cpu(src)[cpu(order).long()[:k]][:, :roww]
    assert same_bits(dst[:k, :roww], want), 'gather_rows != src[order]'
    assert bool((dst[:k, roww:] == SENT_I).all()) and bool((dst[k:] == SENT_I).all()), 'gather_rows wrote outside its rows'


# ---- CONSOL_AFF ------------------------------------------------------------------------------------------------------------------------
AFF_REGIMES = ('randn0.8', 'video3', 'video8', 'sparse_sel', 'flat', 'far')


def make_consol(seed, regime, n, P):
    """ckey [n,64], cshr [n], csel [n,64], use / life [n]: the candidates of a consolidation.  video3 / video8: a few frames of randn x 3 / x 8
    keys with noisy copies at sigma 0.01 .. 1, shrinkage in [1, 10]."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g)
    csel = torch.rand((n, 64), generator=g)
    cshr = torch.rand((n,), generator=g) * 2 + 1
    if regime in ('video3', 'video8'):
        a = 3.0 if regime == 'video3' else 8.0
        hw = max(1, -(-n // 5))
        base = rn(hw, 64) * a
        copy = torch.arange(n) // hw
        sigma = 10.0 ** (-2 + 2 * (copy.float() / max(1, int(copy.max()))))
        ck = base[torch.arange(n) % hw] + rn(n, 64) * sigma[:, None] * (copy > 0).float()[:, None]
        cshr = torch.rand((n,), generator=g) * 9 + 1
    elif regime == 'flat':
        ck = (rn(1, 64) * 0.8).expand(n, 64).clone()
        cshr = torch.full((n,), 2.0)
    else:
        ck = rn(n, 64) * 0.8
        if regime == 'sparse_sel':
            csel = (torch.rand((n, 64), generator=g) < 0.06).float()
            csel[:, 0] = 1.0
    use, life = torch.rand((n,), generator=g) * 3 + 0.01, torch.floor(torch.rand((n,), generator=g) * 40) + 1
    return dict(ckey=ck.contiguous(), cshr=cshr, csel=csel.contiguous(), use=use, life=life, regime=regime, n=n)


def pick_prototypes(c, P, seed=0):
    """pkey / psel [P,64] gathered from the candidates through the exact ranking (every prototype has S_true = 0 with itself); P > n
    wraps around.  'far': prototype 0 moves 30 away in every channel with selection 1 -- its best similarity is below -150."""
    order, _ = rank_ref(c['use'], c['life'], c['n'])
    idx = order[torch.arange(P) % c['n']]
    pk, pe = c['ckey'][idx].clone(), c['csel'][idx].clone()
    if c['regime'] == 'far':
        pk[0], pe[0] = pk[0] + 30.0, 1.0
    return pk.contiguous(), pe.contiguous(), idx


def consol_aff_true(ck, cs, pk, pe):
    """S_true [P, n], its bound E and the magnitude sum."""
    ck, cs, pk, pe = cpu(ck).double(), cpu(cs).double(), cpu(pk).double(), cpu(pe).double()
    P, n = pk.shape[0], ck.shape[0]
    S = torch.empty((P, n), dtype=F64)
    for p0 in range(0, P, 16):
        d = ck[None] - pk[p0:p0 + 16, None]
        S[p0:p0 + 16] = -(pe[p0:p0 + 16, None] * d * d).sum(2) * cs[None] * 0.125
    A = pe @ (ck * ck).t() + 2 * (pe * pk).abs() @ ck.abs().t()
    B = (pe * pk * pk).sum(1)[:, None]
    sc = cs.abs()[None] * 0.125
    bound = sc * (gamma(N_AFF_ACC) * A + gamma(N_AFF_BSQ) * B) + 140 * FTZ * (1 + sc)
    return dict(S=S, bound=bound, mag=sc * (A + B))


def check_consol_aff(S, colmax, true, n, P, what=''):
    """S [rows >= P, ldS], colmax int32 [>= P] as the launch left them.  Returns the worst |err| / bound."""
    S, keys = cpu(S), keys_of(colmax)
    r = check_bound(S[:P, :n].double(), true['S'], true['bound'], what=what + ' S')
    assert bool((S[:P, n:] == NEG_INF).all()), (what, 'the padding [n, ldS) is not -inf')
    assert bool((S[P:] == SENT_F).all()), (what, 'a row of S past P was written')
    stored = S[:P, :n].max(1).values
    dec = key2f(keys[:P])
    assert bool((dec == stored).all()), (what, 'colmax does not decode to the maximum of the stored row', int((dec != stored).sum()))
    assert bool((cpu(colmax)[P:] == SENT_I).all()), (what, 'colmax past P was written')
    return r


# ---- CONSOL_READ ------------------------------------------------------------------------------------------------------------------------
VALUE_KINDS = ('randn', 'x64', 'sparse', 'const')


def make_values(seed, kind, n, C):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn((n, C), generator=g)
    if kind == 'x64':
        v = v * 64
    elif kind == 'sparse':                                                    # mostly exact zeros, per-channel scales 2^-6 .. 2^6
        v = (v - 0.9).clamp(min=0) * torch.exp2(torch.rand((C,), generator=g) * 12 - 6)
    elif kind == 'const':                                                     # constant per channel: a weighted mean of it is that constant
        v = v[:1].expand(n, C).clone()
    return v.to(BF16)


def hand_S(kind, n, P, ldS):
    """Hand-built similarities with the exact keys of their row maxima.  'onehot': candidate (7 p) % n at -3 - p, all others 110 .. 150 below;
    'ramp': 0 down to -120 across the row (through the denormal and zero range of expf), rotated by p."""
    S = torch.full((P, ldS), NEG_INF)
    i = torch.arange(n)
    for p in range(P):
        if kind == 'onehot':
            S[p, :n] = -3.0 - p - 110.0 - (i % 41).float()
            S[p, (7 * p) % n] = -3.0 - p
        else:
            S[p, :n] = -120.0 * (((i + 3 * p) % n).float() / max(1, n - 1))
    return S, torch.from_numpy(f2key(S[:, :n].max(1).values).view(np.int32).copy())


def read_counts(ldS):
    nchunk = -(-ldS // 256)
    return 2 * min(ldS, 256) + nchunk, min(ldS, 256) // 4 + 2 + nchunk, nchunk


def read_rel(ldS):
    na, nz, _ = read_counts(ldS)
    relN = (1 + REL_EXP) * (1 + U_BF16 ** 2) * (1 + gamma(na)) - 1
    zeta = (1 + REL_EXP) * (1 + gamma(nz)) - 1
    theta = (1 + 2 * U32) * (1 + U32) - 1
    phi = (theta + zeta) / (1 - zeta)
    relS = (1 + REL_EXP) * (1 + gamma(nz + 1)) - 1
    phis = (2 * U32 + zeta) / (1 - zeta)
    return relN * (1 + phi) + phi, relS * (1 + phis) + phis


def consol_read_ref(S, colmax, values, cshr, n, P, src, ldS, wrel=None):
    """From the S [>= P, ldS] and colmax a launch reads and the bank rows [src, src + n) of every object: prototypes y [K, P, C] with their
    bound, out_shr [P] with its bound.  wrel [P, n]: a relative change of every NORMALISED weight that the logits' own error adds (chain_ref)."""
    S32 = cpu(S)[:P, :n].contiguous().numpy()
    m = key2f(keys_of(colmax)[:P]).numpy()
    with np.errstate(all='ignore'):
        d = (S32 - m[:, None]).astype(np.float32)
    w = torch.from_numpy(np.exp(d.astype(np.float64)))
    return _read_from_weights(w, values, cshr, n, src, ldS, wrel)


def _read_from_weights(w, values, cshr, n, src, ldS, wrel=None):
    z = w.sum(1, keepdim=True)
    wn = w / z
    moved = wn if wrel is None else wn * (1 + wrel)
    rel_y, rel_s = read_rel(ldS)
    ys, ybs = [], []
    for v in values:
        V = cpu(v)[src:src + n].double()
        y = wn @ V
        e = (moved @ V.abs()) * rel_y + FTZ * (V.abs().sum(0)[None] / z) * 2 + 4 * FTZ
        if wrel is not None:
            e = e + (wn * wrel) @ V.abs()
        ys.append(y)
        ybs.append(e + U_BF16 * (y.abs() + e))
    cs = cpu(cshr)[:n].double()
    shr = wn @ cs
    sb = (moved @ cs.abs()) * rel_s + 4 * FTZ * (1 + cs.abs().sum() / z[:, 0])
    if wrel is not None:
        sb = sb + (wn * wrel) @ cs.abs()
    return dict(y=torch.stack(ys), ybound=torch.stack(ybs), shr=shr, sbound=sb, w=wn, z=z[:, 0])


def check_consol_read(banks, before, out_shr, ref, P, dst, what=''):
    """banks / before: every object's bank after / before the launch.  Returns (worst y ratio, worst out_shr ratio)."""
    ry = 0.0
    for o, (b, b0) in enumerate(zip(banks, before)):
        b, b0 = cpu(b), cpu(b0)
        ry = max(ry, check_bound(b[dst:dst + P].double(), ref['y'][o], ref['ybound'][o], what=f'{what} prototypes of object {o}'))
        assert same_bits(b[:dst], b0[:dst]) and same_bits(b[dst + P:], b0[dst + P:]), (what, o, 'a bank row outside [dst, dst + P) changed')
    osh = cpu(out_shr)
    rs = check_bound(osh[:P].double().view(-1, 1), ref['shr'].view(-1, 1), ref['sbound'].view(-1, 1), what=what + ' out_shr')
    assert bool((osh[P:] == SENT_F).all()), (what, 'out_shr past P was written')
    return ry, rs


# ---- the chain ----------------------------------------------------------------------------------------------------------------------------
def chain_ref(c, values, P):
    """_consolidate in float64: order (exact), prototypes of the values and of the shrinkage with their bounds against the truth."""
    order, q = rank_ref(c['use'], c['life'], P)
    assert distinct_at(q, P), 'the P-th and (P+1)-th quotients tie: choose another seed'
    pk, pe = c['ckey'][order], c['csel'][order]
    t = consol_aff_true(c['ckey'], c['cshr'], pk, pe)
    S, E = t['S'], t['bound']
    w = torch.exp(S - S.max(1, keepdim=True).values)
    wn = w / w.sum(1, keepdim=True)
    Dp, Dm = (wn * torch.exp(E)).sum(1, keepdim=True), (wn * torch.exp(-E)).sum(1, keepdim=True)
    wrel = torch.maximum(torch.exp(E) / Dm - 1, 1 - torch.exp(-E) / Dp)
    n = c['n']
    r = _read_from_weights(w, values, c['cshr'], n, 0, O.OpList.consol_lds(n), wrel)
    r.update(order=order, S=S, E=E)
    return r


# ---- USAGE_TICK -----------------------------------------------------------------------------------------------------------------------------
FX_EDGES = [0, 1, 2 ** 40, 2 ** 40 + 2 ** 16 + 1, 2 ** 53 - 1, 2 ** 53 + 2 ** 29 + 1, 2 ** 63 + 2 ** 39 + 1, 2 ** 64 - 1]


def fx_to_f32(d):
    """The correctly rounded (nearest, ties to even) fp32 of d / 2^40 for a Python integer 0 <= d < 2^64, from the exact rational."""
    if d == 0:
        return np.float32(0.0)
    x = Fraction(d, 2 ** 40)
    e = d.bit_length() - 1 - 40                                               # 2^e <= x < 2^(e+1)
    q = x / Fraction(2) ** (e - 23)                                           # significand in [2^23, 2^24)
    s = q.numerator // q.denominator
    rem = q - s
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and s % 2 == 1):
        s += 1
    return np.float32(math.ldexp(s, e - 23))                                  # (s <= 2^24 and the exponent is far from both ends: exact)


def fx_values(seed, n):
    g = torch.Generator().manual_seed(seed)
    v = list(FX_EDGES) + [int(a) * 2 ** 32 + int(b) for a, b in torch.randint(0, 2 ** 32, (max(0, n - len(FX_EDGES)), 2), generator=g).tolist()]
    return v[:n]


def u64_tensor(vals):
    return torch.from_numpy(np.array(vals, dtype=np.uint64).view(np.int64).copy())


def tick_ref(life, n):
    a = cpu(life).numpy().astype(np.float32).copy()
    a[:n] = a[:n] + np.float32(1.0)
    return torch.from_numpy(a)


def tick_use_ref(use, delta, n, fx):
    a = cpu(use).numpy().astype(np.float32).copy()
    if fx:
        dv = np.array([fx_to_f32(int(v)) for v in cpu(delta).numpy().view(np.uint64)[:n]], dtype=np.float32)
    else:
        dv = cpu(delta).numpy().astype(np.float32)[:n]
    a[:n] = a[:n] + dv
    return torch.from_numpy(a)


# ---- SUMMARIZE / ADD_PE ---------------------------------------------------------------------------------------------------------------------
SUM_REGIMES = ('plain', 'large', 'hard')
REL_W = (1 + 7 * U32) * (1 + U32) ** 2 - 1


def make_summarize(seed, regime, K, HW, C, Q=16):
    g = torch.Generator().manual_seed(seed)
    feat, wl, m = torch.randn((K, HW, C), generator=g), torch.randn((K, HW, Q), generator=g) * 2, torch.rand((K, HW), generator=g)
    if regime == 'large':                                                     # logits +-90: e^-wl overflows / sigma underflows; features x 2^6
        wl = torch.where(torch.rand((K, HW, Q), generator=g) < 0.3, torch.sign(wl) * 90.0, wl)
        feat = feat * 64
    elif regime == 'hard':                                                    # m exactly 0 / 1: object 0 all 1, object 1 all 0, the rest mixed
        m = (m < 0.5).float()
        m[0] = 1.0
        if K > 1:
            m[1] = 0.0
    return feat, wl.contiguous(), m.contiguous()


def summarize_ref(feat, wl, m, HW):
    """y [K, Q, C + 1] (the area in the last column) with its bound, from the stored features (bf16 or fp32), logits and masks."""
    f, wl, m = cpu(feat).double(), cpu(wl).double(), cpu(m).double()[..., None]
    Q = wl.shape[-1]
    m32 = cpu(m).float()
    one_minus = (1.0 - m32).double()                                          # fl(1 - m): exact where m is 0 or 1, one rounding (in rw) elsewhere
    mq = torch.cat([m.expand(-1, -1, Q // 2), (1.0 - m).expand(-1, -1, Q // 2)], -1)
    hard0 = torch.cat([(m == 0).expand(-1, -1, Q // 2), (one_minus == 0).expand(-1, -1, Q // 2)], -1)
    w = torch.sigmoid(wl) * mq
    wb = torch.where(hard0, torch.zeros_like(w), REL_W * w + 2 * FTZ)
    ns = 36 + -(-HW // 128)
    sums = torch.einsum('kpq,kpc->kqc', w, f)
    mag = torch.einsum('kpq,kpc->kqc', w, f.abs())
    sb = ((1 + gamma(ns)) * (1 + REL_W) - 1) * mag + (1 + gamma(ns)) * torch.einsum('kpq,kpc->kqc', wb - REL_W * w, f.abs())
    area, ab = w.sum(1), ((1 + gamma(ns)) * (1 + REL_W) - 1) * w.sum(1) + (1 + gamma(ns)) * (wb - REL_W * w).sum(1)
    y, b = torch.cat([sums, area[..., None]], -1), torch.cat([sb, ab[..., None]], -1)
    exact0 = torch.cat([mag, area[..., None]], -1) == 0
    return dict(y=y, bound=torch.where(exact0, torch.zeros_like(b), b + ns * FTZ), exact0=exact0)


def check_summarize(y, ref, what=''):
    y = cpu(y)
    K = y.shape[0]
    z = ref['exact0']
    assert bool((y[z] == 0).all()), (what, 'a sum of exact zero weights is not an exact zero')
    b = torch.where(z, torch.ones_like(ref['bound']), ref['bound'])
    return check_bound(y.double().reshape(K, -1), ref['y'].reshape(K, -1), b.reshape(K, -1), what=what)


def add_pe_ref(x, pe):
    y = cpu(x).double() + cpu(pe).double()[None]
    return y, U32 * y.abs() + U_BF16 * (y.abs() * (1 + U32)) + 2 * FTZ


# ---- the shared case list ----------------------------------------------------------------------------------------------------------------
# (n, k, usage kind, words cleared)
RANK_CASES = [(1, 1, 'random', 300), (2, 1, 'equal', 5), (2, 2, 'pairs', 5), (17, 1, 'zeros', 5), (17, 8, 'fresh', 5), (17, 17, 'pairs', 5),
              (255, 128, 'random', 5), (256, 256, 'equal', 5), (257, 1, 'big', 5), (257, 128, 'fresh', 5), (1000, 128, 'zeros', 30),
              (1000, 1000, 'random', 5), (4100, 128, 'pairs', 5), (4100, 4100, 'big', 5), (8100, 128, 'fresh', 128)]
# (n, P, regime)
AFF_CASES = [(1, 1, 'randn0.8'), (1, 136, 'video3'), (31, 15, 'video8'), (32, 16, 'video3'), (33, 17, 'sparse_sel'), (33, 1, 'far'), (270, 65, 'video8'),
             (270, 128, 'flat'), (270, 16, 'far'), (1000, 136, 'video3'), (1000, 128, 'video8'), (1000, 17, 'randn0.8'), (31, 128, 'sparse_sel')]
# (n, P, C, K, S kind, value kind, adjacent)
READ_CASES = [(1, 1, 128, 1, 'randn0.8', 'randn', True), (32, 16, 256, 2, 'video3', 'x64', False), (33, 17, 384, 1, 'video8', 'sparse', True),
              (255, 128, 256, 1, 'onehot', 'randn', False), (256, 129, 128, 2, 'ramp', 'x64', True), (257, 136, 256, 1, 'video8', 'const', False),
              (513, 16, 256, 5, 'flat', 'randn', True), (513, 17, 128, 1, 'far', 'sparse', False), (1000, 128, 256, 2, 'video3', 'randn', True),
              (1000, 136, 384, 1, 'ramp', 'sparse', False), (33, 1, 256, 1, 'onehot', 'x64', True), (1000, 129, 128, 1, 'sparse_sel', 'const', False),
              (255, 16, 256, 1, 'flat', 'const', False), (8100, 128, 256, 3, 'video8', 'randn', True)]
# (n, P, K, regime, seed, keep): the chain of _compress on one bank
CHAIN_CASES = [(270, 16, 1, 'randn0.8', 1, 70), (300, 128, 2, 'video3', 2, 100), (513, 17, 1, 'video8', 3, 35), (257, 8, 3, 'sparse_sel', 4, 0)]
BW_WORDS = [0, 1, 255, 256, 257, 1023, 1024, 1025, 131072 + 5]
# (six copies | two fills) of one launch; past 131072 words the grid is capped at 128 blocks and the stride loop takes a second pass
BW_LAUNCHES = [[0, 1, 255, 256, 257, 1023, 1024, 1025], [131072 + 5, 1025, 1024, 1, 257, 255, 131072 + 5, 0], [1023, 1, 1, 256, 1025, 131072 + 5, 1, 255]]
# (nA, nB, nU, fixed point, clear, the absent range)
TICK_CASES = [(255, 256, 257, True, True, None), (257, 255, 256, True, False, None), (256, 257, 255, False, False, None), (300, 1, 17, True, True, 'A'),
              (1, 300, 17, True, False, 'B'), (17, 1, 300, False, False, 'U'), (5, 600, 40, True, True, 'U'), (0, 0, 40, True, True, None)]
# (K, HW, C, regime, fp32 features read out of one buffer with the logits)
SUM_CASES = [(1, 1, 64, 'plain', False), (3, 4, 64, 'hard', True), (1, 127, 256, 'large', False), (3, 128, 64, 'plain', True), (1, 129, 64, 'hard', False),
             (3, 1025, 64, 'large', True), (1, 1620, 256, 'plain', True), (3, 1620, 64, 'hard', False)]


def run_rank_case(dev, execute, n, k, kind, nzero):
    use, life = make_usage(n + k, kind, n)
    g = torch.Generator().manual_seed(n)
    srcs = [torch.randint(-2 ** 31, 2 ** 31 - 1, (n, w), generator=g, dtype=I64).to(I32) for w in (4, 64)]
    b = Bufs(dev)
    order = b.output('order', (k + 5,), I32)
    side = [b.output(f'side{a}', (k + 2, s.shape[1]), I32) for a, s in enumerate(srcs)]
    cleared = b.output('cleared', (nzero + 7,), I32)
    scratch = b.output('scratch', (O.OpList.RS_SPLIT * n,), I32)
    d_srcs = [b.operand(s) for s in srcs]
    ol = O.OpList()
    ol.rank_select(b.operand(use), b.operand(life), order, n=n, k=k, scratch=scratch, gathers=[(d_srcs[0], side[0], 16), (d_srcs[1], side[1], 256)],
                   zero=(cleared, nzero))
    gs = []
    for rowb, kk in ((4, k), (256, k), (512, 1)):                               # GATHER_ROWS through the same order: strides larger than the row
        roww, ssw, dsw = rowb // 4, rowb // 4 + 3, rowb // 4 + 5
        src = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, ssw), generator=g, dtype=I64).to(I32)
        if rowb == 256:
            src[:, :64] = srcs[1]
        dst = b.output(f'gather{rowb}', (kk + 1, dsw), I32)
        ol.gather_rows(b.operand(src), order, dst, k=kk, rowbytes=rowb, src_stride=4 * ssw, dst_stride=4 * dsw)
        gs.append((dst, src, kk, roww))
    execute(ol, b)
    check_rank(dict(order=order, side=side, cleared=cleared), dict(use=use, life=life, srcs=srcs, nzero=nzero), n, k)
    for dst, src, kk, roww in gs:
        check_gather(dst, src, order, kk, roww)
    assert same_bits(side[1][:k], gs[1][0][:k, :64]), 'the side gather of RANK_SELECT differs from GATHER_ROWS through the same order'
    assert b.guards_intact()


def aff_buffers(b, n, P):
    ldS = O.OpList.consol_lds(n)
    S = b.output('S', (P + 2, ldS), F32)
    cm0 = torch.full((P + 3,), SENT_I, dtype=I32)
    cm0[:P] = 0
    return S, b.output('colmax', (P + 3,), I32, cm0), ldS


def run_aff_case(dev, execute, n, P, regime, seed=None):
    c = make_consol(1000 * n + P if seed is None else seed, regime, n, P)
    pk, pe, _ = pick_prototypes(c, P)
    b = Bufs(dev)
    S, colmax, ldS = aff_buffers(b, n, P)
    ol = O.OpList()
    ol.consol_aff(b.operand(c['ckey']), b.operand(c['cshr']), b.operand(pk), b.operand(pe), S, colmax, n=n, P=P)
    execute(ol, b)
    true = consol_aff_true(c['ckey'], c['cshr'], pk, pe)
    assert bool(torch.isfinite(true['S']).all()) and bool(torch.isfinite(true['bound']).all())
    if regime == 'far':
        assert float(true['S'][0].max()) < -150
    r = check_consol_aff(S, colmax, true, n, P, what=f'consol_aff {regime} n={n} P={P}')
    assert b.guards_intact()
    return dict(S=r), dict(c=c, pk=pk, pe=pe, true=true, S=cpu(S), colmax=cpu(colmax))


class ReadCase:
    """The buffers of one CONSOL_READ: K banks of T rows, NaN everywhere except the candidates' rows [src, src + n)."""

    def __init__(self, dev, b, n, P, C, K, vkind, adjacent, seed):
        self.n, self.P, self.C, self.K = n, P, C, K
        self.dst = 3
        self.src = self.dst + P if adjacent else self.dst + P + 37
        T = self.src + n + 2
        self.before = []
        for o in range(K):
            bank = torch.full((T, C), float('nan'), dtype=BF16)
            bank[self.src:self.src + n] = make_values(seed + o, vkind, n, C)
            self.before.append(bank)
        self.banks = [b.output(f'bank{o}', (T, C), BF16, bank) for o, bank in enumerate(self.before)]
        self.vptrs = b.operand(torch.tensor([v.data_ptr() for v in self.banks], dtype=I64))
        self.scratch = b.output('part', (O.OpList.consol_scratch_floats(n, P, C, K),), F32)
        self.out_shr = b.output('out_shr', (P + 2,), F32)

    def launch(self, ol, S, colmax, cshr):
        ol.consol_read(S, colmax, self.vptrs, cshr, self.scratch, self.out_shr, n=self.n, P=self.P, C=self.C, K=self.K, src=self.src, dst=self.dst)


def run_read_case(dev, execute, n, P, C, K, skind, vkind, adjacent):
    seed = 7 * n + P + C + K
    b = Bufs(dev)
    ol = O.OpList()
    if skind in ('onehot', 'ramp'):
        ldS = O.OpList.consol_lds(n)
        S0, cm0 = hand_S(skind, n, P, ldS)
        S, colmax = b.operand(S0), b.operand(cm0)
        g = torch.Generator().manual_seed(seed)
        cshr = torch.rand((n,), generator=g) * 9 + 1
    else:
        c = make_consol(seed, skind, n, P)
        pk, pe, _ = pick_prototypes(c, P)
        S, colmax, ldS = aff_buffers(b, n, P)
        cshr = c['cshr']
        ol.consol_aff(b.operand(c['ckey']), b.operand(cshr), b.operand(pk), b.operand(pe), S, colmax, n=n, P=P)
    rc = ReadCase(dev, b, n, P, C, K, vkind, adjacent, seed)
    rc.launch(ol, S, colmax, b.operand(cshr))
    execute(ol, b)
    what = f'consol_read {skind}/{vkind} n={n} P={P} C={C} K={K}'
    ref = consol_read_ref(S, colmax, rc.before, cshr, n, P, rc.src, ldS)
    for t in (ref['y'], ref['ybound'], ref['shr'], ref['sbound']):
        assert bool(torch.isfinite(t).all()), (what, 'a reference or bound is not finite')
    ry, rs = check_consol_read(rc.banks, rc.before, rc.out_shr, ref, P, rc.dst, what)
    if skind == 'onehot':                                                       # the prototype IS the candidate's stored row
        hot = (7 * torch.arange(P)) % n
        for o in range(K):
            assert same_bits(rc.banks[o][rc.dst:rc.dst + P], rc.before[o][rc.src + hot]), (what, 'one-hot prototype != the stored row')
        assert same_bits(rc.out_shr[:P], cshr[hot]), (what, 'one-hot out_shr != the shrinkage')
    if skind == 'flat':
        assert bool((ref['z'] == n).all())
    assert b.guards_intact()
    return dict(y=ry, out_shr=rs), dict(rc=rc, S=cpu(S), colmax=cpu(colmax), cshr=cshr, ref=ref, ldS=ldS)


def run_chain_case(dev, execute, n, P, K, regime, seed, keep):
    """One bank laid out like a Bucket: long-term rows [0, L), working rows from ws = L; n candidates + keep newer tokens.  Every array has a
    few rows behind the working tokens, and the long-term region more than P free rows, that must stay as they were."""
    c = make_consol(seed, regime, n, P)
    C, n_long, L = 256, 5, 5 + P + 4
    ws, T = L, L + n + keep + 3
    g = torch.Generator().manual_seed(seed + 50)
    tot = n + keep
    rawkey, rawsel, rawshr = torch.randn((T, 64), generator=g), torch.rand((T, 64), generator=g), torch.rand((T,), generator=g) + 1
    use, life = torch.rand((T,), generator=g), torch.floor(torch.rand((T,), generator=g) * 9) + 1
    rawkey[ws:ws + n], rawsel[ws:ws + n], rawshr[ws:ws + n], use[ws:ws + n], life[ws:ws + n] = c['ckey'], c['csel'], c['cshr'], c['use'], c['life']
    vals = [torch.randn((T, C), generator=g).to(BF16) for _ in range(K)]
    for o in range(K):
        vals[o][ws:ws + n] = make_values(seed + o, VALUE_KINDS[(seed + o) % 4], n, C)
    Ahi0, Alo0, sc0 = torch.randn((T, 128), generator=g).to(BF16), torch.randn((T, 128), generator=g).to(BF16), torch.rand((T,), generator=g)
    b = Bufs(dev)
    names = dict(rawkey=rawkey, rawsel=rawsel, rawshr=rawshr, use=use, life=life, Ahi=Ahi0, Alo=Alo0, scale=sc0)
    names.update({f'val{o}': v for o, v in enumerate(vals)})
    d = {k: b.output(k, tuple(v.shape), v.dtype, v) for k, v in names.items()}
    vptrs = b.operand(torch.tensor([d[f'val{o}'].data_ptr() for o in range(K)], dtype=I64))
    order, psel = b.output('order', (P + 2,), I32), b.output('psel', (P + 1, 64), F32)
    S, colmax, ldS = aff_buffers(b, n, P)
    part = b.output('part', (O.OpList.consol_scratch_floats(n, P, C, K),), F32)
    dst = n_long
    ol = O.OpList()
    ol.rank_select(d['use'][ws:], d['life'][ws:], order, n=n, k=P, scratch=b.output('scratch', (O.OpList.RS_SPLIT * n,), I32),
                   gathers=[(d['rawkey'][ws:], d['rawkey'][dst:], 256), (d['rawsel'][ws:], psel, 256)], zero=(colmax, P))
    ol.consol_aff(d['rawkey'][ws:], d['rawshr'][ws:], d['rawkey'][dst:], psel, S, colmax, n=n, P=P)
    ol.consol_read(S, colmax, vptrs, d['rawshr'][ws:], part, d['rawshr'][dst:], n=n, P=P, C=C, K=K, src=ws, dst=dst)
    ol.key_prep(d['rawkey'][dst:], d['rawshr'][dst:], d['Ahi'][dst:], d['Alo'][dst:], d['scale'][dst:], n=P, query=False)
    arrays = [(d[k], names[k][0].numel() * names[k].element_size()) for k in names]
    fills = [(d['use'][dst:], P, 0), (d['life'][dst:], P, LIFE_EPS_BITS)]
    copies = [(t[ws + n:], t[ws:], rb * keep) for t, rb in arrays] if keep > 0 else []
    assert keep <= n
    ol.bank_write(copies, fills)
    execute(ol, b)
    what = f'chain {regime} n={n} P={P} K={K}'
    ref = chain_ref(c, [v[ws:ws + n] for v in vals], P)
    ratios = {}
    got = {k: cpu(v) for k, v in d.items()}
    assert torch.equal(cpu(order)[:P].long(), ref['order']) and bool((cpu(order)[P:] == SENT_I).all()), (what, 'order')
    rows = slice(dst, dst + P)
    assert same_bits(got['rawkey'][rows], c['ckey'][ref['order']]) and same_bits(cpu(psel)[:P], c['csel'][ref['order']]), (what, 'prototype keys / selections')
    ratios['S'] = check_consol_aff(S, colmax, dict(S=ref['S'], bound=ref['E']), n, P, what)
    for o in range(K):
        ratios['chain_y'] = max(ratios.get('chain_y', 0.0), check_bound(got[f'val{o}'][rows].double(), ref['y'][o], ref['ybound'][o], what=f'{what} values {o}'))
    ratios['chain_shr'] = check_bound(got['rawshr'][rows].double().view(-1, 1), ref['shr'].view(-1, 1), ref['sbound'].view(-1, 1), what=what + ' shrinkage')
    kp = key_prep_ref(got['rawkey'][rows], got['rawshr'][rows], False)
    ratios['key_prep'] = check_key_prep(got['Ahi'][rows], got['Alo'][rows], got['scale'][rows], kp, what + ' key_prep')
    assert bool((got['use'][rows] == 0).all()) and bool((bits(got['life'][rows]) == LIFE_EPS_BITS).all()), (what, 'counters of the new prototypes')
    for k, v0 in names.items():
        gk = got[k]
        assert same_bits(gk[ws:ws + keep], v0[ws + n:ws + n + keep]), (what, k, 'the kept working tokens were not moved to the region start')
        assert same_bits(gk[:dst], v0[:dst]) and same_bits(gk[dst + P:ws], v0[dst + P:ws]), (what, k, 'a long-term row outside the new prototypes changed')
        assert same_bits(gk[ws + keep:], v0[ws + keep:]), (what, k, 'a row behind the moved tokens changed')
    assert same_bits(got['rawsel'][rows], rawsel[rows]), (what, 'the selections of the long-term rows are not kept: nothing writes them')
    assert b.guards_intact()
    return ratios


def run_tick_case(dev, execute, nA, nB, nU, fx, clear, absent):
    g = torch.Generator().manual_seed(nA * 7 + nB * 3 + nU + fx)
    lifeA, lifeB = torch.floor(torch.rand((nA + 6,), generator=g) * 50), torch.floor(torch.rand((nB + 6,), generator=g) * 50) + 1e-7
    lifeA[0] = 2.0 ** 24                                                        # adding 1 changes nothing
    use = torch.rand((nU + 6,), generator=g) * 4
    if fx:
        delta = u64_tensor(fx_values(nU, nU + 6))
    else:
        delta = torch.rand((nU + 6,), generator=g)
    b = Bufs(dev)
    dA, dB, dU, dD = b.output('lifeA', (nA + 6,), F32, lifeA), b.output('lifeB', (nB + 6,), F32, lifeB), b.output('use', (nU + 6,), F32, use), \
        b.output('delta', (nU + 6,), delta.dtype, delta)
    ol = O.OpList()
    ol.usage_tick(None if absent == 'A' else dA, nA, None if absent == 'B' else dB, nB, None if absent == 'U' else dU, dD, nU, delta_fx=fx, clear_delta=clear)
    execute(ol, b)
    what = f'tick nA={nA} nB={nB} nU={nU} fx={fx} clear={clear} absent={absent}'
    assert same_bits(dA, lifeA if absent == 'A' else tick_ref(lifeA, nA)), (what, 'life A')
    assert same_bits(dB, lifeB if absent == 'B' else tick_ref(lifeB, nB)), (what, 'life B')
    assert same_bits(dU, use if absent == 'U' else tick_use_ref(use, delta, nU, fx)), (what, 'use')
    want_d = delta.clone()
    if fx and clear and absent != 'U':
        want_d[:nU] = 0
    assert same_bits(dD, want_d), (what, 'delta')
    assert b.guards_intact()


def run_bank_write_case(dev, execute, words):
    """Six copies and two fills of different sizes in ONE launch; a null source with non-zero words is skipped."""
    g = torch.Generator().manual_seed(sum(words))
    b = Bufs(dev)
    copies, fills, checks = [], [], []
    for s, w in enumerate(words[:6]):
        src = torch.randint(-2 ** 31, 2 ** 31 - 1, (max(w, 1),), generator=g, dtype=I64).to(I32)
        dst = b.output(f'dst{s}', (w + 3,), I32)
        copies.append((b.operand(src), dst, 4 * w))
        checks.append((dst, src, w))
    for t, (w, pat) in enumerate(zip(words[6:8], (0, LIFE_EPS_BITS))):
        dst = b.output(f'fill{t}', (w + 3,), I32)
        fills.append((dst, w, pat))
    ol = O.OpList()
    ints, ptrs = [0] * 10, [0] * 14
    for s, (src, dst, nb) in enumerate(copies):
        ints[s], ptrs[2 * s], ptrs[2 * s + 1] = nb // 4, src, dst
    skipped = None
    if words[0] == 0:                                                           # slot 0: a null source with non-zero words
        skipped = copies[0][1]
        ints[0], ptrs[0] = 77, None
    for t, (dst, w, pat) in enumerate(fills):
        ints[6 + t], ints[8 + t], ptrs[12 + t] = w, pat, dst
    ol.add(O.BANK_WRITE, 0, ints, [], ptrs)
    execute(ol, b)
    for dst, src, w in checks:
        gd = cpu(dst)
        assert same_bits(gd[:w], src[:w]) and bool((gd[w:] == SENT_I).all()), ('bank_write copy', w)
    if skipped is not None:
        assert bool((cpu(skipped) == SENT_I).all())
    for (dst, w, pat) in fills:
        gd = cpu(dst)
        assert bool((gd[:w] == pat).all()) and bool((gd[w:] == SENT_I).all()), ('bank_write fill', w)
    assert b.guards_intact()


CAST_EDGES = [0.0, -0.0, float('inf'), float('-inf'), float('nan'), 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -9,
              2.0 ** -130, -2.0 ** -133, 3 * 2.0 ** -134, 2.0 ** -126 * (1 - 2.0 ** -9), 3.3e38, 3.4e38, -65280.0, 2.0 ** -149]


def run_misc_case(dev, execute, n):
    """COPY2D, MEMSET32, CAST both ways and AXPY at n elements (n around one block)."""
    g = torch.Generator().manual_seed(n)
    b = Bufs(dev)
    ol = O.OpList()
    rows, roww, ssw, dsw = n, 3, 5, 4
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (rows, ssw), generator=g, dtype=I64).to(I32)
    c2 = b.output('copy2d', (rows, dsw), I32)
    ol.copy2d(b.operand(src), c2, rows=rows, rowbytes=4 * roww, src_stride=4 * ssw, dst_stride=4 * dsw)
    ms = b.output('memset', (n + 5,), I32)
    ol.memset32(ms, n, LIFE_EPS_BITS)
    x32 = torch.randn((n,), generator=g) * torch.exp2(torch.randint(-20, 20, (n,), generator=g).float())
    e = torch.tensor(CAST_EDGES, dtype=F32)
    x32[:min(n, e.numel())] = e[:n]
    xb = (torch.randn((n,), generator=g) * 3).to(BF16)
    xb[:min(n, e.numel())] = e[:n].to(BF16)
    if n > 20:
        xb[18:20] = torch.tensor([0x0001, 0x807f - 0x10000], dtype=torch.int16).view(BF16)     # bf16 denormals
    to_b, to_f = b.output('to_bf16', (n + 3,), BF16), b.output('to_f32', (n + 3,), F32)
    ol.cast(b.operand(x32), to_b, n=n)
    ol.cast(b.operand(xb), to_f, n=n, to_f32=True)
    ax, ay = torch.randn((n,), generator=g) * 100, torch.randn((n,), generator=g)
    y = b.output('axpy', (n + 3,), F32, torch.cat([ay, torch.full((3,), SENT_F)]))
    a = 0.3
    ol.axpy(b.operand(ax), y, n=n, a=a)
    execute(ol, b)
    g2 = cpu(c2)
    assert same_bits(g2[:, :roww], src[:, :roww]) and bool((g2[:, roww:] == SENT_I).all()), 'copy2d'
    gm = cpu(ms)
    assert bool((gm[:n] == LIFE_EPS_BITS).all()) and bool((gm[n:] == SENT_I).all()), 'memset32'
    gb, wb = cpu(to_b)[:n], x32.to(BF16)
    nan = torch.isnan(wb.float())
    assert torch.equal(torch.isnan(gb.float()), nan) and same_bits(gb[~nan], wb[~nan]) and bool((cpu(to_b)[n:] == SENT_F).all()), 'cast to bf16'
    gf, wf = cpu(to_f)[:n], xb.float()
    nan = torch.isnan(wf)
    assert torch.equal(torch.isnan(gf), nan) and same_bits(gf[~nan], wf[~nan]) and bool((cpu(to_f)[n:] == SENT_F).all()), 'cast to f32'
    want = (np.float32(a) * ax.numpy()).astype(np.float32) + ay.numpy()
    assert same_bits(cpu(y)[:n], torch.from_numpy(want.astype(np.float32))) and bool((cpu(y)[n:] == SENT_F).all()), 'axpy'
    assert b.guards_intact()


def run_summarize_case(dev, execute, K, HW, C, regime, f32_form, partials=False):
    Q = 16
    feat, wl, m = make_summarize(HW + C + K, regime, K, HW, C)
    b = Bufs(dev)
    ol = O.OpList()
    nchunk = -(-HW // 128)
    y = b.output('y', (K, Q, C + 1), F32)
    scratch = b.output('scratch', (K, nchunk, Q, C + 1), F32)
    d_m = b.operand(m)
    if f32_form:                                                               # [feature | logits] rows of C + Q fp32 values in one buffer
        both = b.operand(torch.cat([feat, wl], -1).contiguous())
        ol.summarize(both, both.view(-1)[C:], d_m, y, K=K, HW=HW, C=C, Q=Q, scratch=scratch, feat_f32=True, ldf=C + Q, ldw=C + Q)
        stored = feat
    else:
        stored = feat.to(BF16)
        ol.summarize(b.operand(stored), b.operand(wl), d_m, y, K=K, HW=HW, C=C, Q=Q, scratch=scratch)
    execute(ol, b)
    ref = summarize_ref(stored, wl, m, HW)
    assert bool(torch.isfinite(ref['y']).all()) and bool(torch.isfinite(ref['bound']).all())
    r = check_summarize(y, ref, what=f'summarize {regime} K={K} HW={HW} C={C} f32={f32_form}')
    if partials:                                                               # the final sums are the chunk-ordered sum of the kernel's own partials
        part, acc = cpu(scratch), np.zeros((K, Q, C + 1), dtype=np.float32)
        for ch in range(nchunk):
            acc = acc + part[:, ch].numpy()
        assert same_bits(y, torch.from_numpy(acc)), 'summarize: the final sums are not the chunk-ordered sum of the partials'
    assert b.guards_intact()
    return r


def run_add_pe_case(dev, execute, B, n8):
    n = 8 * n8
    g = torch.Generator().manual_seed(B + n8)
    x, pe = (torch.randn((B, n), generator=g) * 4).to(BF16), (torch.randn((n,), generator=g) * 4).to(BF16)
    pe[0] = -x[0, 0]                                                            # an exact cancellation
    b = Bufs(dev)
    y = b.output('y', (B, n), BF16)
    ol = O.OpList()
    ol.add_pe(b.operand(x), b.operand(pe), y, B=B, n=n)
    execute(ol, b)
    want, bound = add_pe_ref(x, pe)
    r = check_bound(cpu(y).double(), want, bound, what=f'add_pe B={B} n8={n8}')
    assert b.guards_intact()
    return r
