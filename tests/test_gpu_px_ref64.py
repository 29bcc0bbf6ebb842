"""The mask decoder's pixel kernels (csrc/elementwise.hip) on the MI355X against the float64 references of tests/px_ref64.py, element by
element: one launch (for a chain the shortest launch sequence) per form and case of the list shared with tests/test_px_ref64_cpu.py, every
output pre-filled with NaN between sentinel elements that must survive, every value within its derived bound, every exact property asserted
as exact, a second run of the same launches bit-identical, and every bit-identity that the comments of elementwise.hip promise between two
forms asserted as such (fused against two launches, four pixels against one, compile-time against run-time K and r, shared against per-lane
aggregation, clips in lock step and mixed counts against each clip alone, AREA_DOWN3 against three AREA_DOWNs, gru4 against gru, UP4_SOFTMAX's
mask-down outputs against a separate MASK_DOWN).  The A/B forms are reached through the descriptor's flags, never through the environment.
Each test prints its worst |err| / bound ("px_ref64 ratio ..."); DESIGN.md keeps the table."""
import pytest
import torch

import px_ref64 as P
from cutie_amd import _lib
from cutie_amd import ops as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32, BF16 = torch.float32, torch.bfloat16


def launch(ol):
    ex, arr = _lib.HipExecutor(), ol.finalize()

    def run():
        ex.run(arr)
        torch.cuda.synchronize()
    run()
    return run


@pytest.mark.parametrize('case', P.ALL_CASES, ids=P.case_id)
def test_kernel_within_the_float64_bound(case):
    op, kw = case
    ratios = P.RUNNERS[op][0](DEV, launch, **kw)
    assert P.show(op, kw, ratios) <= 1.0


# ---- what the launcher refuses: an error and no launch -------------------------------------------------------------------------------
def _refused(ol, b, match):
    with pytest.raises(RuntimeError, match=match):
        _lib.HipExecutor().run(ol.finalize())
    torch.cuda.synchronize()
    for n in b.outs:
        assert bool(torch.isnan(b[n].float()).all()), (n, 'a refused launch wrote something')
    assert b.guards_intact()


def test_up4_softmax_refuses_17_planes():
    b = P.Bufs(DEV)
    x = b.operand(torch.zeros((16, 2, 2)))
    prob, lup = P.out_nan(b, 'prob', (17, 8, 8)), P.out_nan(b, 'lup', (17, 8, 8))
    ol = O.OpList()
    ol.up4_softmax(x, prob, lup, P=17, h=2, w=2, from_logits=True)
    _refused(ol, b, 'up4_softmax')


def test_up4_softmax_refuses_a_mixed_launch_with_the_run_time_object_count():
    counts, h, w = (1, 3), 4, 4
    b = P.Bufs(DEV)
    x = b.operand(torch.zeros((4, h, w)))
    prob = P.out_nan(b, 'prob', (6, 4 * h, 4 * w))
    ol = O.OpList()
    ol.add(O.UP4_SOFTMAX, 1 | 8, [max(counts) + 1, h, w, 0, len(counts), O.pack_counts(counts)], [], [x, prob, None])
    _refused(ol, b, 'mixed form')


@pytest.mark.parametrize('ints', [(4, 3, 120), (4, -1, 120), (4, 2, 10)], ids=['B%Kg', 'Kg<0', 'stride'])
def test_upsample2x_add_refuses_bad_groups(ints):
    B, kg, stride = ints
    h, w, C = 2, 2, 8
    b = P.Bufs(DEV)
    g, skip = b.operand(torch.zeros((B, h, w, C), dtype=BF16)), b.operand(torch.zeros((4, 200, C), dtype=BF16))
    y = P.out_nan(b, 'y', (B, 2 * h, 2 * w, C), BF16)
    ol = O.OpList()
    ol.add(O.UPSAMPLE2X_ADD, 0, [B, h, w, C, kg, stride], [], [g, skip, y])
    _refused(ol, b, 'upsample2x_add')


def test_upsample2x_add_refuses_mixed_counts_that_do_not_add_up():
    B, h, w, C = 4, 2, 2, 8
    b = P.Bufs(DEV)
    g, skip = b.operand(torch.zeros((B, h, w, C), dtype=BF16)), b.operand(torch.zeros((4, 200, C), dtype=BF16))
    y = P.out_nan(b, 'y', (B, 2 * h, 2 * w, C), BF16)
    ol = O.OpList()
    ol.add(O.UPSAMPLE2X_ADD, 0, [B, h, w, C, 0, 20, O.pack_counts((1, 2))], [], [g, skip, y])
    _refused(ol, b, 'mixed form')


def test_eca_head_refused_at_other_channel_counts():
    B, HW, C = 1, 5, 128
    b = P.Bufs(DEV)
    x = b.operand(torch.zeros((B, HW, C), dtype=BF16))
    part, wk = b.operand(torch.zeros((B, 1, C))), b.operand(torch.zeros(5))
    pw = b.operand(torch.zeros(256, dtype=BF16))
    y, plog = P.out_nan(b, 'y', (B, HW, C), BF16), P.out_nan(b, 'plog', (B, HW))
    ol = O.OpList()
    ol.add(O.ECA_APPLY, 0, [B, HW, C], [], [x, None, wk, x, y, part, pw, None, plog])
    _refused(ol, b, 'eca')


@pytest.mark.parametrize('C', [24, 40, 264])
def test_gap_refuses_channel_counts_its_block_cannot_split(C):
    b = P.Bufs(DEV)
    x = b.operand(torch.zeros((1, 4, C), dtype=BF16))
    y, part = P.out_nan(b, 'y', (1, C)), P.out_nan(b, 'part', (1, 1, C))
    ol = O.OpList()
    ol.gap(x, y, B=1, HW=4, C=C, scratch=part)
    _refused(ol, b, 'gap')
