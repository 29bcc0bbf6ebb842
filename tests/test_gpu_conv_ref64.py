"""Every conv launch the plans really make, against the float64 reference (tests/ref64.py), element by element.

Five scenarios are recorded through the executor (a first frame, a propagated frame with the look-ahead window of the image encoder, a
memory frame, a plain propagated frame): the base model at 480p with 1 and 3 objects and at 1080p with 5 objects (long-term memory on),
cutie-small at 480p with 3 objects, and 4 clips x 3 objects in lock step.  Every unique CONV launch -- (i[0:22], flags, f0, f1), with the
tile (i17) and split-K (i19) the plans chose -- is replayed once per operand regime with the recorded packed weights and bias and fresh
activations:
  * 'randn'  -- randn * 0.5 for the inputs and the residual;
  * 'sparse' -- post-ReLU inputs with per-channel scales log-uniform in [2^-6, 2^6] and a residual of randn * 128.
Guard bands: x1 / x2 / the residual sit between NaN rows, the unused channels of an ldx > C or ldr > Cout row and the rows between the
clips' residual maps are NaN (a read outside the operand, or a padded lane multiplied by a zero weight, gives a NaN); y sits between
sentinel rows and its ldy > Cout gap columns hold the sentinel too (the arena packs unrelated tensors side by side: every sentinel must
survive).  The GAP side job stays on: its accumulator must be the per-value fixed point of the stored outputs, exactly.
"""
import collections
import json
import os
import pytest
import torch

import ref64 as R
from cutie_amd import _lib, ops as O
from cutie_amd.config import default_config

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
SENT16 = 0x7F81                      # a signalling-NaN pattern no conv stores (its NaNs are quiet, 0x7FC0)
SENT32 = 0x7F800001
FRAMES = 15
DEV = 'cuda'
TILE_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'cutie_amd', 'tiles_gfx950.json')


class _Rec:
    """Executor shim that records every descriptor array of a run (as in test_gpu_parity.py)."""
    def __init__(self, ex):
        self.ex, self.rec, self.is_mock = ex, [], ex.is_mock

    def run(self, arr):
        self.rec.append(arr.copy())
        self.ex.run(arr)

    def stream(self):
        return self.ex.stream()

    def time_ops(self, arr, iters):
        return self.ex.time_ops(arr, iters)


def family(tile):
    if tile == O.COUT1_TILE:
        return 'cout1'
    if tile in O.PC_HALO:
        return 'pc-halo'
    if tile in O.PC_TILES:
        return 'pc-stream'
    if tile in O.DMA_TILES:
        return 'dma'
    return 'igemm'


class _Weights:
    """Device tensors of an engine's packed weights, found by address (a launch's p2 / p3 may point inside one)."""
    def __init__(self, eng):
        self.spans = []
        seen = set()

        def add(t):
            if isinstance(t, torch.Tensor) and t.device.type == DEV and t.numel():
                key = (t.data_ptr(), t.numel())
                if key not in seen:
                    seen.add(key)
                    self.spans.append((t.data_ptr(), t.numel() * t.element_size(), t))

        def walk(v, depth):
            if isinstance(v, torch.Tensor):
                add(v)
            elif isinstance(v, dict) and depth < 3:
                for u in v.values():
                    walk(u, depth + 1)
            elif isinstance(v, (list, tuple)) and depth < 3:
                for u in v:
                    walk(u, depth + 1)
            elif hasattr(v, '__slots__') and depth < 3 and not isinstance(v, type):
                for s in v.__slots__:
                    walk(getattr(v, s, None), depth + 1)
        walk(eng.w, 0)
        for k, v in eng.__dict__.items():
            if k not in ('w', '_plans', 'pool') and isinstance(v, (torch.Tensor, dict)):
                walk(v, 0)

    def find(self, ptr, nbytes, dtype):
        for base, size, t in self.spans:
            if base <= ptr and ptr + nbytes <= base + size:
                flat = t.reshape(-1).view(torch.uint8)
                return flat[ptr - base:ptr - base + nbytes].view(dtype)
        return None

    def inside(self, ptr, nbytes):
        return any(base <= ptr and ptr + nbytes <= base + size for base, size, _ in self.spans)


def _guarded(gen, rows, C, ld, regime, scale=0.5, pad_rows=None):
    """bf16 operand of `rows` rows of ld values (channels [C, ld) NaN) between NaN guard bands; returns (buffer, interior view)."""
    guard = max(4096, 2 * ld)
    buf = torch.full((2 * guard + rows * ld,), float('nan'), dtype=BF16, device=DEV)
    inner = buf[guard:guard + rows * ld].view(rows, ld)
    inner.copy_(R.operand(gen, rows, C, regime=regime, ld=ld, scale=scale, fill=float('nan')))
    if pad_rows is not None:
        inner[pad_rows] = float('nan')
    return buf, inner


def replay(one, wts, regime, seed, ex=None):
    """Replay one recorded CONV descriptor (a one-record array) with fresh operands; check it against ref64.  Returns the worst
    |err| / bound."""
    rec = one[0]
    i, flags, f, p = rec['i'], int(rec['flags']), rec['f'], [int(v) for v in rec['p']]
    g = R.ConvGeom.from_desc(i, flags, f)
    tile, splitk, nzero = int(i[17]), int(i[19]), int(i[21])
    cpad = -(-g.Cout // 128) * 128
    w = wts.find(p[2], cpad * g.Kpad * 2, BF16)
    assert w is not None, 'packed weights of the launch not found among the engine tensors'
    bias = wts.find(p[3], g.Cout * 4, F32) if p[3] else None
    assert bias is not None or not p[3]
    gen = torch.Generator(device=DEV).manual_seed(seed)
    npx = g.B * g.H * g.W
    xb1, x1 = _guarded(gen, npx, g.C1, g.ldx1, regime)
    xb2, x2 = _guarded(gen, npx, g.C2, g.ldx2, regime) if g.C2 else (None, None)
    rb = r = None
    if p[4]:
        n = g.res_extent()
        gaps = None
        if g.res_bcast and g.f0 > 0:                                   # rows between the clips' maps: not read
            m = torch.arange(n, device=DEV)
            gaps = (m % g.f1) >= g.OHW
        rb, r = _guarded(gen, n, g.Cout, g.ldr, regime, scale=0.5 if regime == 'randn' else 128.0, pad_rows=gaps)
    f32 = g.out_f32
    guard = max(4096, 2 * g.ldy)
    ydt, sent, ivt = (F32, SENT32, torch.int32) if f32 else (BF16, SENT16, torch.int16)
    ybuf = torch.empty((2 * guard + g.M * g.ldy,), dtype=ydt, device=DEV)
    ybuf.view(ivt).fill_(sent - (1 << 32) if sent >= (1 << 31) else sent)
    gap = torch.zeros((g.B, g.Cout), dtype=torch.int64, device=DEV) if p[7] else None
    zbuf = torch.full((max(nzero, 1),), 12345, dtype=torch.int64, device=DEV) if p[8] else None
    one = one.copy()
    P = one['p'][0]
    P[0] = x1.data_ptr()
    P[1] = x2.data_ptr() if x2 is not None else 0
    P[4] = r.data_ptr() if r is not None else 0
    P[5] = ybuf.data_ptr() + guard * ybuf.element_size()
    P[6] = O.splitk_scratch(DEV).data_ptr()
    assert int(i[20]) * 1024 <= O.splitk_scratch(DEV).numel()
    P[7] = gap.data_ptr() if gap is not None else 0
    P[8] = zbuf.data_ptr() if zbuf is not None else 0
    for q, nb in ((9, 22), (10, 23)):                                   # next-weights touch: keep it where it names live weights
        if P[q] and not wts.inside(int(P[q]), int(i[nb])):
            P[q], one['i'][0, nb] = 0, 0
    (ex or _lib.HipExecutor()).run(one)
    if DEV == 'cuda':
        torch.cuda.synchronize()
    what = f'tile {tile} splitk {splitk} {regime} i={[int(v) for v in i[:17]]} flags={flags} f={[float(v) for v in f[:2]]}'
    iv = ybuf.view(ivt)
    s = sent - (1 << 32) if sent >= (1 << 31) else sent
    assert bool((iv[:guard] == s).all()) and bool((iv[guard + g.M * g.ldy:] == s).all()), what + ': write outside y'
    y = ybuf[guard:guard + g.M * g.ldy].view(g.M, g.ldy)
    if g.ldy > g.Cout:
        assert bool((y.view(ivt)[:, g.Cout:] == s).all()), what + ': write into the ldy > Cout gap'
    bm = O.ALL_TILES[tile][0] if tile in O.ALL_TILES else None
    rows = R.sample_rows(g, bm=bm, halo=O.PC_HALO.get(tile), n_random=2048, seed=seed, device=DEV)
    y64, bound = R.conv_ref64(g, x1, w, x2=x2, bias=bias, res=r, rows=rows)
    worst = R.check_bound(y[rows, :g.Cout], y64, bound, what)
    if zbuf is not None:
        assert bool((zbuf[:nzero] == 0).all()), what + ': zero job'
    if gap is not None:
        st = y[:, :g.Cout].to(torch.float64).view(g.B, g.OHW, g.Cout)
        exact = R.gap_fixed(st).sum(1) * 16
        assert torch.equal(gap, exact), what + ': GAP accumulator differs from the fixed point of the stored values in %d of %d' % (
            int((gap != exact).sum()), gap.numel())
        if bool((st.abs() <= R.GAP_LIMIT).all()):
            mean = st.mean(1)
            got = gap.to(torch.float64) * 2.0 ** -24 / g.OHW
            assert bool(((got - mean).abs() <= 2.0 ** -21 + 2.0 ** -24 * mean.abs()).all()), what + ': GAP mean'
    return worst


def _record(run):
    real = _lib.get_executor()
    rec = _Rec(real)
    _lib.set_executor_for_testing(rec)
    try:
        with torch.inference_mode():
            run()
        if DEV == 'cuda':
            torch.cuda.synchronize()
    finally:
        _lib.set_executor_for_testing(None)
    return rec.rec


def _core_run(net, h, w, K, cfg_kw, seed):
    from cutie_amd.inference.inference_core import InferenceCore
    from cutie_amd.utils.synth import SyntheticClip

    def run():
        clip = SyntheticClip(h, w, K, FRAMES, seed=seed)
        fr = [clip.frame(t).to(DEV) for t in range(FRAMES)]
        proc = InferenceCore(net, cfg=default_config(**cfg_kw))
        proc.step(fr[0], clip.first_mask().to(DEV), objects=clip.objects)       # first frame (memorised)
        proc.step(fr[1], next_images=fr[2:14])                                    # propagated, encoder window of 12 frames
        proc.step(fr[2], next_images=fr[3:15])                                    # memory frame (mem_every = 2)
        proc.step(fr[3], end=True)
    return run


def _lockstep_run(net, C, K, cfg_kw):
    from cutie_amd.inference.lockstep import LockstepCores
    from cutie_amd.utils.synth import SyntheticClip

    def run():
        clips = [SyntheticClip(480, 854, K, FRAMES, seed=60 + c) for c in range(C)]
        fr = [[cl.frame(t).to(DEV) for t in range(FRAMES)] for cl in clips]
        ls = LockstepCores(net, default_config(**cfg_kw), C)
        ls.step([f[0] for f in fr], [cl.first_mask().to(DEV) for cl in clips], [cl.objects for cl in clips])
        ls.step([f[1] for f in fr], next_images=[f[2:14] for f in fr])
        ls.step([f[2] for f in fr], next_images=[f[3:15] for f in fr])
        ls.step([f[3] for f in fr], end=True)
    return run


SCENARIOS = ['base_480p_k1', 'base_480p_k3', 'base_1080p_k5', 'small_480p_k3', 'lockstep_4x3_480p']
LT = dict(use_long_term=True, mem_every=2)


@pytest.fixture(scope='module')
def census():
    """scenario -> list of (record, weights) of the CONV launches first seen in that scenario, plus per-scenario tile counts."""
    from cutie_amd.model.cutie import CUTIE
    from cutie_amd.utils.synth_weights import make_state_dict as mk, MODEL_CFG_SMALL
    from oracle.weights import make_state_dict
    _lib.set_executor_for_testing(None)
    base = CUTIE(default_config()).to(DEV).eval()
    base.load_weights(make_state_dict(seed=0))
    small = CUTIE(default_config(model='small')).to(DEV).eval()
    small.load_weights(mk(seed=0, m=MODEL_CFG_SMALL))
    runs = {'base_480p_k1': (base, _core_run(base, 480, 854, 1, LT, 1)),
            'base_480p_k3': (base, _core_run(base, 480, 854, 3, LT, 2)),
            'base_1080p_k5': (base, _core_run(base, 1080, 1920, 5, LT, 3)),
            'small_480p_k3': (small, _core_run(small, 480, 854, 3, dict(LT, model='small'), 4)),
            'lockstep_4x3_480p': (base, _lockstep_run(base, 4, 3, LT))}
    table = {tuple(k): tuple(v) for k, v in json.load(open(TILE_TABLE))['tiles']}
    seen, out = set(), {}
    for name in SCENARIOS:
        net, run = runs[name]
        arrs = _record(run)
        wts = _Weights(net.engine())
        mine, new, alts = {}, [], []
        for arr in arrs:
            for n in range(len(arr)):
                if int(arr['kind'][n]) != O.CONV:
                    continue
                fl = int(arr['flags'][n])
                key = tuple(int(v) for v in arr['i'][n][:22]) + (fl, float(arr['f'][n][0]), float(arr['f'][n][1]))
                if key in mine:
                    continue
                mine[key] = int(arr['i'][n][17])
                if key not in seen:
                    seen.add(key)
                    new.append((arr[n:n + 1].copy(), wts))
                    # the table's own entry for this geometry, where a class-tied entry (the batched twin of a one-frame plan) overrode it
                    i = arr['i'][n]
                    alt = table.get((int(i[0]) * int(i[7]) * int(i[8]), int(i[9]), int(i[3]) + int(i[4]), int(i[11]), int(i[13]), fl & 3, int(i[1]), int(i[2])))
                    side = arr['p'][n, 7] or arr['p'][n, 8]
                    if alt and alt[0] != int(i[17]) and (not side or alt[0] in O.DMA_TILES or alt[0] in O.PC_TILES):
                        one = arr[n:n + 1].copy()
                        one['i'][0, 17], one['i'][0, 19] = alt
                        alts.append((one, wts))
        out[name] = dict(new=new, alts=alts, tiles=mine, nets=(base, small))
    return out


@pytest.mark.parametrize('name', SCENARIOS)
def test_every_recorded_conv_launch_against_float64(census, name):
    sc = census[name]
    per = collections.Counter(family(t) for t in sc['tiles'].values())
    checked, worst, bad = collections.Counter(), 0.0, []
    for k, (rec, wts) in enumerate(sc['new'] + sc['alts']):
        for regime in ('randn', 'sparse'):
            try:
                worst = max(worst, replay(rec, wts, regime, seed=1000 * k + (regime == 'sparse')))
            except AssertionError as e:                                  # (every launch is checked; the failures are listed together)
                bad.append(str(e).split('\n')[0])
        checked[family(int(rec['i'][0, 17]))] += 1
    print(f'\n{name}: {len(sc["tiles"])} unique conv launches {dict(per)}; replayed here (first seen in this scenario) '
          f'{sum(checked.values()) - len(sc["alts"])} {dict(checked)} (with {len(sc["alts"])} table entries overridden by a class-tied one, tiles '
          f'{sorted({int(r["i"][0, 17]) for r, _ in sc["alts"]})}); worst |err| / bound {worst:.3f}; tiles {sorted(set(sc["tiles"].values()))}')
    assert not bad, f'{len(bad)} failing replays:\n' + '\n'.join(bad[:40])
    assert sum(checked.values()) == len(sc['new']) + len(sc['alts'])


def test_recorded_launches_cover_the_chosen_tiles(census):
    """Every tile id the plans chose was replayed above, the pair-step tile 146 among them; pair-step tile 142 is the table's entry for the
    12-frame encoder window's e_proj (M = 19440), which the class-tied entry of the window (the one-frame plan's K order) overrides in a
    frame: it is replayed on that recorded launch as the table's alternate.  The tiles of the packaged table that no scenario reaches are
    listed."""
    chosen, replayed, alts = set(), set(), set()
    for name in SCENARIOS:
        chosen |= set(census[name]['tiles'].values())
        replayed |= {int(rec['i'][0, 17]) for rec, _ in census[name]['new']}
        alts |= {int(rec['i'][0, 17]) for rec, _ in census[name]['alts']}
    assert chosen == replayed
    assert 146 in chosen and 142 in alts, (sorted(chosen), sorted(alts))
    table = {int(v[0]) for _, v in json.load(open(TILE_TABLE))['tiles']}
    print(f'\ntiles chosen: {sorted(chosen)}\ntable alternates replayed: {sorted(alts - chosen)}\n'
          f'table tiles no scenario reaches: {sorted(table - chosen - alts)}')
