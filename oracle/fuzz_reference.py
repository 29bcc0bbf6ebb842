"""Differential fuzz of the oracle against the EXECUTED reference: random event scripts (objects added over time, deletions,
re-specified masks, soft float masks, permanent commits, update_config, clear_* calls, end flag; random memory settings incl.
long-term memory and object chunks) are run through the unmodified reference InferenceCore and through OracleProcessor with
the same weights; per-frame probabilities and memory-bank sizes must agree.  Complements the fixed golden scenarios
(tests/golden): those travel to the GPU box, this runs only where /root/reference exists (the build container).

    python oracle/fuzz_reference.py --seeds 0 1 2 [--frames 14] [--model small]
    python oracle/fuzz_reference.py --seeds 5 8 20 --record tests/golden/fuzz_reference_seeds_5_8_20.npz

--record also stores the reference's per-frame probabilities (whole frames, on a grid of 1/PROB_LEVELS: pack_probs) and memory
sizes of every seed it could run, for tests/test_fuzz_cpu.py to hold the oracle to without the reference checkout.

TEST INFRASTRUCTURE (see oracle/__init__.py)."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
from oracle.make_golden import _wrap, import_reference, memory_sizes, reference_cfg      # noqa: E402

PROB_LEVELS = 1023                     # --record: probabilities p in [0, 1] stored as round(p * PROB_LEVELS)


def pack_probs(p):
    """(planes, H, W) probabilities -> uint8 (2, planes, H, W): round(p * PROB_LEVELS), differenced along W and then H, zigzag-coded,
    low and high byte.  Compressed, the differences take less than half the room of the plain levels."""
    x = np.round(np.asarray(p, dtype=np.float64) * PROB_LEVELS).astype(np.int32)
    d = np.diff(np.diff(x, axis=-1, prepend=0), axis=-2, prepend=0)
    z = (d << 1) ^ (d >> 31)
    return np.stack([z & 255, z >> 8]).astype(np.uint8)


def unpack_probs(b):
    """pack_probs(p) -> p on the grid of 1/PROB_LEVELS (float64; within 0.5 / PROB_LEVELS of p)."""
    z = b[0].astype(np.int32) | (b[1].astype(np.int32) << 8)
    d = (z >> 1) ^ -(z & 1)
    return np.cumsum(np.cumsum(d, axis=-2), axis=-1) / PROB_LEVELS


def random_scenario(seed, frames):
    from oracle.scenarios import LT_SMALL
    r = np.random.Generator(np.random.PCG64(seed))
    k = int(r.integers(2, 5))
    cfg = dict(mem_every=int(r.integers(2, 4)), max_mem_frames=int(r.integers(2, 4)), stagger_updates=int(r.choice([1, 2, 5])))
    if r.random() < 0.4:
        cfg.update(use_long_term=True, long_term=dict(LT_SMALL))
    if r.random() < 0.3:
        cfg['chunk_size'] = int(r.integers(1, 3))
    sc = dict(cfg=cfg, kind='synth', h=int(r.choice([80, 96, 100])), w=int(r.choice([112, 120, 136])), k=k, frames=frames, sub=2,
              add_at={}, delete_at={}, float_mask_at=[], end_at=[], permanent_at=[], update_config_at={},
              clear_non_permanent_at=[], repropagate_at=[], clear_memory_at=[])
    first = int(r.integers(1, k + 1))
    alive, unseen, deleted = list(range(1, first + 1)), list(range(first + 1, k + 1)), False
    sc['add_at'][0] = list(alive)
    if r.random() < 0.3:
        sc['float_mask_at'].append(0)
    for t in range(1, frames):
        u = r.random()
        if u < 0.12 and unseen:                                   # new objects, optionally together with known ones
            n_new = int(r.integers(1, len(unseen) + 1))
            new, unseen = unseen[:n_new], unseen[n_new:]
            known = [o for o in alive if r.random() < 0.4]
            sc['add_at'][t] = known + new                          # tmp-id order: known objects first (object_manager.py:53)
            alive += new
        elif u < 0.20 and len(alive) > 1:
            victim = int(r.choice(alive))
            alive.remove(victim)
            deleted = True
            sc['delete_at'][t] = [victim]
        elif u < 0.28:                                             # every known object re-specified (need_segment False)
            sc['add_at'][t] = list(alive)
            if r.random() < 0.4 and not deleted and alive == list(range(1, len(alive) + 1)):
                sc['float_mask_at'].append(t)
            if r.random() < 0.5:
                sc['permanent_at'].append(t)
        elif u < 0.33:
            sc['update_config_at'][t] = dict(mem_every=int(r.integers(2, 5)))
        elif u < 0.38:
            sc['clear_non_permanent_at'].append(t)
        elif u < 0.43 and not deleted and alive == list(range(1, len(alive) + 1)):
            sc['repropagate_at'].append(t)                         # clear_sensory_memory + previous soft output as the mask
        elif u < 0.46:
            sc['clear_memory_at'].append(t)
            sc['add_at'][t] = list(alive)
    if r.random() < 0.5:
        sc['end_at'].append(frames - 1)
    # drawn last so that the event scripts of earlier seeds stay what they were
    if r.random() < 0.2:
        cfg['flip_aug'] = True
        # flip_aug (batch of 2) together with object chunks is not comparable: MaskDecoder.forward concatenates the per-chunk
        # logits [bs*chunk,1,H,W] along dim 0 and then views them as [bs, K, H, W] (big_modules.py:300-302), which for bs = 2
        # interleaves the flipped and the plain lane across objects -- the reference's own output is scrambled there
        # (seeds 55 and 67 found it: max |dprob| 0.4 against the oracle, which decodes each lane on its own)
        cfg.pop('chunk_size', None)
    if r.random() < 0.25 and sc['h'] > 80:
        cfg['max_internal_size'] = 80                              # shorter side 96 / 100 -> internal resize path, still >= 30 tokens
                                                                   # (with fewer than top_k tokens the reference's topk raises)
    if r.random() < 0.5 and frames > 4:
        # memory limits changed mid-clip (the GUI's working / long-term memory sliders go through update_config,
        # gui/main_controller.py:518-560): the token limits are re-derived at the next memory frame (memory_manager.py:228-235)
        t = int(r.integers(2, frames - 1))
        over = sc['update_config_at'].setdefault(t, {})
        if cfg.get('use_long_term'):
            mx = int(r.integers(3, 7))
            lt = dict(cfg['long_term'], max_mem_frames=mx, min_mem_frames=int(r.integers(2, mx)),
                      max_num_tokens=int(r.choice([24, 40, 64])), buffer_tokens=int(r.choice([4, 12])))
            over['long_term'] = lt
        else:
            over['max_mem_frames'] = int(r.integers(2, 6))
    return sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seeds', type=int, nargs='+', default=[0, 1, 2])
    ap.add_argument('--frames', type=int, default=14)
    ap.add_argument('--tol', type=float, default=5e-3)
    ap.add_argument('--model', default='base', choices=['base', 'small'], help='cutie/config/model/{base,small}.yaml')
    ap.add_argument('--record', default=None, help='.npz: the reference\'s probabilities and memory sizes of every seed it ran')
    args = ap.parse_args()
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    CUTIE, InferenceCore = import_reference()
    from oracle import scenarios as S
    from oracle.inference import DEFAULT_CFG, OracleProcessor
    from oracle.net import OracleNet
    from oracle.weights import MODEL_CFG, MODEL_CFG_SMALL, make_state_dict
    mcfg = MODEL_CFG_SMALL if args.model == 'small' else MODEL_CFG
    sd = make_state_dict(seed=0, m=mcfg)
    net = CUTIE(reference_cfg(args.model)).eval()
    net.load_weights({k: v.clone() for k, v in sd.items()})
    onet = OracleNet(sd, mcfg)
    wrap = lambda over: reference_cfg(args.model, **{k: (_wrap(v) if isinstance(v, dict) else v) for k, v in over.items()})
    bad = 0
    rec = {'frames': np.int64(args.frames), 'model': np.array(args.model), 'seeds': []}
    for seed in args.seeds:
        sc = random_scenario(seed, args.frames)
        S.SCENARIOS['_fuzz'] = sc
        rs, os_ = [], []
        try:
            routs, _ = S.run_scenario(lambda over: InferenceCore(net, cfg=wrap(over)), '_fuzz',
                                      record=lambda t, p: rs.append(memory_sizes(p)), make_cfg=wrap)
        except Exception as e:                                     # the script trips a bug of the reference itself: not comparable
            print(f'seed {seed}: skipped, the reference raised {type(e).__name__}: {e}')
            continue
        rec['seeds'].append(seed)
        rec[f'sizes_{seed}'] = np.array(rs, dtype=np.int64)
        for t, p in enumerate(routs):
            rec[f'prob_{seed}_{t}'] = pack_probs(p.numpy())

        def osizes(p):
            w = sum(p.work.size(b) for b in p.work.buckets)
            pe = sum(p.work.perm_end[b] for b in p.work.buckets)
            lt = sum(p.long.size(b) for b in p.long.buckets) if p.use_long_term else 0
            return [w, pe, lt, len(p.work.buckets)]

        oouts, _ = S.run_scenario(lambda over: OracleProcessor(onet, dict(DEFAULT_CFG, **over)), '_fuzz',
                                  record=lambda t, p: os_.append(osizes(p)))
        errs = [float((a - b).abs().max()) if a.shape == b.shape else float('inf') for a, b in zip(routs, oouts)]
        ok = rs == os_ and max(errs) < args.tol
        bad += not ok
        events = {k: v for k, v in sc.items() if k.endswith('_at') and v}
        brief = {k: v for k, v in sc['cfg'].items() if k != 'long_term'}
        print(f'seed {seed}: {"ok " if ok else "FAIL"} max|dprob| {max(errs):.2e} sizes_equal {rs == os_} {sc["h"]}x{sc["w"]} k={sc["k"]} cfg {brief} {events}')
        if not ok:
            print('   per-frame errors', [f'{e:.1e}' for e in errs])
            print('   ref sizes   ', rs)
            print('   oracle sizes', os_)
    if args.record:
        rec['seeds'] = np.array(rec['seeds'], dtype=np.int64)
        np.savez_compressed(args.record, **rec)
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
