"""Random event scripts (oracle/fuzz_reference.py::random_scenario: objects added over time, deletions, re-specified / soft
masks, permanent commits, update_config, clear_* calls, end flag, random memory settings incl. long-term memory and chunks).

  * oracle vs the EXECUTED reference: its probabilities and memory sizes on three scripts, recorded by oracle/fuzz_reference.py --record
    (tests/golden/fuzz_reference_seeds_5_8_20.npz);
  * product (descriptor interpreter) vs oracle."""
import os

import numpy as np
import pytest
import torch

from cutie_amd import _lib
from cutie_amd.config import default_config
from oracle import scenarios as S
from oracle.fuzz_reference import PROB_LEVELS, random_scenario, unpack_probs
from oracle.inference import OracleProcessor, DEFAULT_CFG
from oracle.weights import make_state_dict

from mock_exec import MockExecutor

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
FUZZ_GOLD = os.path.join(ROOT, 'tests', 'golden', 'fuzz_reference_seeds_5_8_20.npz')


def test_oracle_matches_recorded_reference_on_random_scripts(oracle_net):
    """Seeds 5, 8, 20 (object chunks + re-propagation; long-term memory + internal resize + float masks + permanent memory; flip_aug):
    per-frame probabilities within 2e-3 of the executed reference's (less the recording's rounding) and memory-bank sizes equal, frame by
    frame.  The record: `python oracle/fuzz_reference.py --seeds 5 8 20 --tol 2e-3 --record <npz>` (live agreement 1.6e-6)."""
    gold = np.load(FUZZ_GOLD)
    frames = int(gold['frames'])
    assert str(gold['model']) == 'base' and gold['seeds'].tolist() == [5, 8, 20]
    for seed in gold['seeds'].tolist():
        S.SCENARIOS['_fuzz'] = random_scenario(seed, frames)
        sizes = []
        try:
            outs, _ = S.run_scenario(lambda over: OracleProcessor(oracle_net, dict(DEFAULT_CFG, **over)), '_fuzz',
                                     record=lambda t, p: sizes.append(oracle_sizes(p)))
        finally:
            del S.SCENARIOS['_fuzz']
        assert sizes == gold[f'sizes_{seed}'].tolist(), seed
        assert len(outs) == frames
        for t, o in enumerate(outs):
            ref = unpack_probs(gold[f'prob_{seed}_{t}'])
            assert tuple(o.shape) == ref.shape, (seed, t, tuple(o.shape), ref.shape)
            err = float(np.abs(o.numpy().astype(np.float64) - ref).max())
            assert err < 2e-3 - 0.5 / PROB_LEVELS, (seed, t, err)          # |oracle - reference| < 2e-3


@pytest.fixture(scope='module')
def product_net():
    from cutie_amd.model.cutie import CUTIE
    prev = _lib._executor
    _lib.set_executor_for_testing(MockExecutor())
    net = CUTIE(default_config())
    net.load_weights(make_state_dict(seed=0))
    yield net
    _lib.set_executor_for_testing(prev)


def product_sizes(p):
    m = p.memory
    return [sum(b.n_perm + b.n_work for b in m.buckets.values()), sum(b.n_perm for b in m.buckets.values()),
            sum(b.n_long for b in m.buckets.values()), len(m.buckets)]


def oracle_sizes(p):
    return [sum(p.work.size(b) for b in p.work.buckets), sum(p.work.perm_end[b] for b in p.work.buckets),
            sum(p.long.size(b) for b in p.long.buckets) if p.use_long_term else 0, len(p.work.buckets)]


@pytest.mark.parametrize('seed', [0, 6, 20, 32])      # long-term + chunks; reference-crashing script; flip_aug; internal resize
def test_product_matches_oracle_on_random_scripts(seed, product_net, oracle_net):
    """(seed 6 is a script the reference itself cannot run: deleting the only object of a bucket that holds nothing but
    permanent memory in long-term mode raises KeyError at kv_memory_store.py:300; oracle and product purge it cleanly.)"""
    from cutie_amd.inference.inference_core import InferenceCore
    S.SCENARIOS['_fuzz'] = random_scenario(seed, 14)
    try:
        ps, os_ = [], []
        oouts, _ = S.run_scenario(lambda over: OracleProcessor(oracle_net, dict(DEFAULT_CFG, **over)), '_fuzz',
                                  record=lambda t, p: os_.append(oracle_sizes(p)))
        outs, _ = S.run_scenario(lambda over: InferenceCore(product_net, cfg=default_config(**over)), '_fuzz',
                                 record=lambda t, p: ps.append(product_sizes(p)), make_cfg=lambda over: default_config(**over))
    finally:
        del S.SCENARIOS['_fuzz']
    assert ps == os_
    for t, (p, o) in enumerate(zip(outs, oouts)):
        assert p.shape == o.shape and torch.isfinite(p).all()
        d = (p - o).abs()
        bmax, bmean, _ = S.trajectory_bounds('base')
        assert float(d.max()) < bmax and float(d.mean()) < bmean, (seed, t, float(d.max()), float(d.mean()))


@pytest.mark.parametrize('seed', [201, 216])          # FIFO memory with deletions / re-specified masks; long-term memory + flip_aug
def test_hints_change_nothing_on_random_scripts(seed):
    """The same random event scripts with `next_images` hints on every step (the frames that follow in the script -- wrong ones where
    the script re-propagates or pre-commits) against no hints, through the descriptor interpreter: bit-identical probabilities, with
    the look-ahead lanes on their own streams' bookkeeping and in one lane (Engine.one_lane).  Round 5 ran seeds 200-215 this way."""
    from cutie_amd.inference.inference_core import InferenceCore
    from cutie_amd.model.cutie import CUTIE
    mx = MockExecutor()
    mx.per_sample_conv = True          # (torch's CPU conv may sum differently per batch size; the HIP tiles of one K-order class do not)
    prev = _lib._executor
    _lib.set_executor_for_testing(mx)

    class Hinted:
        def __init__(self, proc, imgs):
            self.__dict__.update(p=proc, imgs=imgs)

        def step(self, img, *a, **k):
            idx = [i for i, x in enumerate(self.imgs) if x is img]
            if idx and not k.get('end') and self.imgs[idx[0] + 1:idx[0] + 9]:
                k['next_images'] = self.imgs[idx[0] + 1:idx[0] + 9]
            return self.p.step(img, *a, **k)

        def __getattr__(self, n):
            return getattr(self.p, n)

        def __setattr__(self, n, v):
            setattr(self.p, n, v)

    S.SCENARIOS['_fuzz'] = random_scenario(seed, 16)
    orig = S.scenario_inputs
    try:
        cache = orig('_fuzz')
        S.scenario_inputs = lambda name: cache        # (the same frame tensors for every run: hints are matched by storage)
        imgs = [st[0] for st in cache[0]]
        net = CUTIE(default_config())
        net.load_weights(make_state_dict(seed=0))
        mk = lambda over: default_config(**over)
        plain, _ = S.run_scenario(lambda over: InferenceCore(net, cfg=mk(over)), '_fuzz', make_cfg=mk)
        for lane in (False, True):
            net.engine().one_lane = lane
            got, _ = S.run_scenario(lambda over: Hinted(InferenceCore(net, cfg=mk(over)), imgs), '_fuzz', make_cfg=mk)
            assert len(got) == len(plain)
            for t, (a, b) in enumerate(zip(got, plain)):
                assert torch.equal(a, b), (seed, lane, t, float((a - b).abs().max()))
    finally:
        S.scenario_inputs = orig
        del S.SCENARIOS['_fuzz']
        _lib.set_executor_for_testing(prev)

