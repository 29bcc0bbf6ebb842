"""Edge / error behaviour of the InferenceCore surface (segment without memory, empty masks, missing `objects`, unsorted object
lists, deleting unknown / all objects, `end` on the first frame, arbitrary object ids, float masks without ids, odd frame
sizes): the outcomes recorded from the EXECUTED reference (oracle/make_edge_cases.py -> tests/golden/edge_cases.json) must be
reproduced by the product (descriptor interpreter on CPU) and by the oracle -- same exception types, same result summaries."""
import json
import os

import pytest

from cutie_amd import _lib
from cutie_amd.config import default_config
from oracle.edge_cases import CASES, run_case
from oracle.inference import OracleProcessor, DEFAULT_CFG
from oracle.weights import make_state_dict

from mock_exec import MockExecutor

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'edge_cases.json')))


@pytest.fixture(scope='module')
def product_net():
    from cutie_amd.model.cutie import CUTIE
    prev = _lib._executor
    _lib.set_executor_for_testing(MockExecutor())
    net = CUTIE(default_config())
    net.load_weights(make_state_dict(seed=0))
    yield net
    _lib.set_executor_for_testing(prev)


from oracle.edge_cases import INTENDED      # where the product deliberately does not reproduce the reference


def test_every_case_is_recorded():
    assert sorted(GOLD) == sorted(CASES)


# (cases whose step raises in the middle of a frame -- e.g. unsorted_new_objects, object_manager.py:53 -- leave that frame's features in the image
# feature store; it says "Leaking ..." when it is dropped, exactly like the reference's store does for the same script, image_feature_store.py:47-49)
@pytest.mark.filterwarnings('ignore:Leaking:UserWarning')
@pytest.mark.parametrize('name', sorted(CASES))
def test_product_reproduces_reference_outcome(name, product_net):
    from cutie_amd.inference.inference_core import InferenceCore
    got = run_case(name, lambda over: InferenceCore(product_net, cfg=default_config(**over)))
    want = INTENDED[name][0] if name in INTENDED else GOLD[name]
    assert got == want, (name, got, want)


@pytest.mark.filterwarnings('ignore:Leaking:UserWarning')           # (the step that raises leaves its frame in the feature store, as above)
def test_consolidation_with_fewer_candidates_than_prototypes_raises(product_net):
    """An 80 x 112 clip has 35 stride-16 cells; with 3 / 2 memory frames a consolidation has 35 candidates for 64 prototypes.  The reference
    raises there (torch.topk, "selected index k out of range", memory_manager.py:339; oracle/inference.py:362 likewise); RANK_SELECT with
    k > n would leave the rest of the order, and the prototypes built from it, to whatever an earlier call left in the buffers.  With 8
    prototypes the same clip consolidates."""
    import torch
    from cutie_amd.inference.inference_core import InferenceCore
    from cutie_amd.utils.synth import SyntheticClip
    from oracle.scenarios import LT_SMALL

    def run(P):
        lt = dict(LT_SMALL, max_mem_frames=3, min_mem_frames=2, num_prototypes=P, max_num_tokens=400, buffer_tokens=100)
        p, c = InferenceCore(product_net, cfg=default_config(mem_every=1, use_long_term=True, long_term=lt)), SyntheticClip(80, 112, 3, 6, seed=7)
        with torch.inference_mode():
            p.step(c.frame(0), c.first_mask(), objects=[1, 2, 3])
            for t in range(1, 6):
                p.step(c.frame(t))
        return p

    with pytest.raises(RuntimeError, match=r'n=35 .*num_prototypes=64'):
        run(64)
    assert max(b.n_long for b in run(8).memory.buckets.values()) >= 8


@pytest.mark.parametrize('name', sorted(CASES))
def test_oracle_reproduces_reference_outcome(name, oracle_net):
    got = run_case(name, lambda over: OracleProcessor(oracle_net, dict(DEFAULT_CFG, **over)))
    if got == ['ok', 'no object manager']:
        pytest.skip('the oracle restates the object manager as a plain id list')
    assert got == GOLD[name], (name, got, GOLD[name])
