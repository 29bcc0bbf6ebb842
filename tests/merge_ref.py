"""numpy model of PROB_TO_ID flags&16 (include/cutie_hip.h, ABI 8): every source resampled bilinearly to the output size in fp32 with
RESIZE's expression order (csrc/elementwise.hip resize_kernel: the same source index, lambdas and order of multiplies and adds; numpy
does not contract), quantised by truncation as (x * 255).to(torch.uint8), summed as integers, first maximum, lut."""
import numpy as np

f32 = np.float32


def _axis(n_in, n_out):
    s = f32(n_in) / f32(n_out)
    f = np.maximum((np.arange(n_out, dtype=f32) + f32(0.5)) * s - f32(0.5), f32(0))
    i0 = np.minimum(f.astype(np.int32), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), (f - i0.astype(f32)).astype(f32)


def resize(prob, OH, OW):
    """fp32 [P, h, w] -> fp32 [P, OH, OW] = RESIZE (flags == 0), bit for bit."""
    prob = np.asarray(prob, dtype=f32)
    P, h, w = prob.shape
    y0, y1, ly = _axis(h, OH)
    x0, x1, lx = _axis(w, OW)
    ly, lx = ly[None, :, None], lx[None, None, :]
    one = f32(1)
    a, b = prob[:, y0][:, :, x0], prob[:, y0][:, :, x1]
    c, d = prob[:, y1][:, :, x0], prob[:, y1][:, :, x1]
    out = (one - ly) * ((one - lx) * a + lx * b) + ly * ((one - lx) * c + lx * d)
    assert out.dtype == f32
    return out


def quantise(x):
    """(x * 255).to(torch.uint8) / numpy astype(uint8): truncation."""
    return (np.asarray(x, dtype=f32) * f32(255)).astype(np.uint8)


def member_scores(probs, OH, OW):
    """Per member the uint8 scores [P, OH, OW] the file route would dump."""
    return [quantise(resize(p, OH, OW)) for p in probs]


def sums(probs, OH, OW):
    return sum(q.astype(np.int32) for q in member_scores(probs, OH, OW))


def merge(probs, lut, OH, OW):
    """-> ids [OH, OW] (int64): lut[first plane with the largest integer sum]."""
    return np.asarray(lut, dtype=np.int64)[np.argmax(sums(probs, OH, OW), axis=0)]


def smooth_probs(P, h, w, seed, smooth=True):
    """Seeded softmax planes (torch, CPU) of the `_probs` kind of tests/test_gpu_egress.py: object-like low-frequency logits, sharpened."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, h, w, generator=g)
    if smooth:
        x = F.interpolate(torch.randn(1, P, max(h // 16, 2), max(w // 16, 2), generator=g), size=(h, w), mode='bicubic', align_corners=False)[0] * 4 + x * 0.3
    return torch.softmax(x, 0)
