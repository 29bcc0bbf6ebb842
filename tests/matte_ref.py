"""Numpy model of PROB_TO_ID flags == 256 / 512 (include/cutie_hip.h ABI 11, forms added, csrc/matte.hip): the visualisation modes, the alpha matte
and the soft masks of the reference's interactive tool (gui/interactive_utils.py:152-229, gui/resource_manager.py:166-173) in float32,
every multiply and add rounded on its own, in the reference's operation order (numpy does not contract).  tests/golden/matte/ holds
what the reference's torch functions write for the same inputs (tools/make_matte_golden.py): the bytes are equal."""
import numpy as np

import merge_ref

f32 = np.float32
HARD_MODES = {'davis': 0, 'light': 1, 'fade': 2}
SOFT_MODES = {'popup': 3, 'layer': 4}
MODE_CODES = {**HARD_MODES, **SOFT_MODES, 'alpha': 5}
ALPHAS = {'davis': 0.5, 'light': 0.9, 'fade': 0.5}


def q8(x):
    """(uint8)(x * 255.0f), the product clamped to [0, 255]."""
    return np.clip(np.asarray(x, dtype=f32) * f32(255), f32(0), f32(255)).astype(np.uint8)


def im_f32(frame):
    """uint8 [H, W, 3] -> float32, v / 255.0f correctly rounded."""
    return np.asarray(frame, dtype=np.uint8).astype(f32) / f32(255)


def planes_at(planes, OH, OW):
    """The planes at the output size: themselves, or RESIZE's (flags == 0) sample."""
    planes = np.asarray(planes, dtype=f32)
    return planes if planes.shape[1:] == (OH, OW) else merge_ref.resize(planes, OH, OW)


def target_sum(planes, targets):
    """m [OH, OW]: the target planes added in list order, starting from the first; 0 for an empty list."""
    m = np.zeros(planes.shape[1:], dtype=f32)
    for j, q in enumerate(targets):
        m = planes[q].copy() if j == 0 else m + planes[q]
    return m


def hard(mode, frame, ids, table):
    """davis / light / fade: frame uint8 [H, W, 3], ids uint8 [H, W], table uint8 [256, 4] -> uint8 [H, W, 3]."""
    im = im_f32(frame)
    alpha = ALPHAS[mode]
    a, b = f32(alpha), f32(1.0 - alpha)
    col = np.asarray(table, dtype=np.uint8)[np.asarray(ids)][..., :3].astype(f32) / f32(255)
    fg = im * a + b * col
    bg = im * f32(0.6) if mode == 'fade' else im
    return q8(np.where((np.asarray(ids) != 0)[..., None], fg, bg))


def popup(frame, m):
    im = im_f32(frame)
    g = ((im[..., 0] * f32(0.3) + im[..., 1] * f32(0.59)) + im[..., 2] * f32(0.11))[..., None]
    m = m[..., None]
    return q8(m * im + (f32(1) - m) * g)


def layer(frame, m, layer_rgba):
    im = im_f32(frame)
    L = np.asarray(layer_rgba, dtype=np.uint8).astype(f32) / f32(255)
    la, lr, m, one = L[..., 3:4], L[..., :3], m[..., None], f32(1)
    x = (im * ((one - m) * (one - la)) + (lr * (one - m)) * la) + im * m
    return q8(np.clip(x, f32(0), f32(1)))


def alpha(m):
    return q8(np.clip(m, f32(0), f32(1)))


def soft(planes, OH, OW):
    """uint8 [P - 1, OH, OW]: the object planes quantised."""
    return q8(planes_at(planes, OH, OW)[1:])


def composite(mode, frame=None, planes=None, targets=(), ids=None, table=None, layer_rgba=None, out_hw=None, want_alpha=False):
    """One launch of the composite stage -> (frame uint8 [OH, OW, 3] or None, matte uint8 [OH, OW] or None)."""
    if mode in HARD_MODES:
        return hard(mode, frame, ids, table), None
    OH, OW = out_hw if out_hw is not None else np.asarray(planes).shape[1:]
    m = target_sum(planes_at(planes, OH, OW), list(targets))
    a = alpha(m) if (want_alpha or mode == 'alpha') else None
    if mode == 'alpha':
        return None, a
    return (popup(frame, m) if mode == 'popup' else layer(frame, m, layer_rgba)), a


class MatteExecutor:
    """Wraps another executor (tests/mock_exec.py's interpreter on host memory, or a wrapper of it) and runs PROB_TO_ID flags == 256 /
    512 through the model: the slots of include/cutie_hip.h ABI 11, forms added.  The PNG stage on its own (flags == 8 without planes), which
    follows them, is served from tests/png_ref.py.  ``log`` keeps what every launch wrote: ('popup', frame, matte, targets) / ('soft', planes)."""
    is_mock = True

    def __init__(self, inner):
        self.inner = inner
        self.composites = self.softs = 0
        self.log = []

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def stream(self):
        return 0

    def run_one(self, rec):
        import ctypes
        import torch
        from mock_exec import view, U8, F32
        flags = int(rec['flags'])
        i, p = [int(v) for v in rec['i']], [int(v) for v in rec['p']]
        if int(rec['kind']) == 36 and flags == 8 and not p[0]:
            import png_ref
            from mock_exec import I32
            data, adler = png_ref.encode(view(p[2], U8, (i[1], i[2])).numpy())
            fits = len(data) <= i[7]
            view(p[4], I32, (4,)).copy_(torch.tensor([len(data), adler - (1 << 32) if adler >= 1 << 31 else adler, 0 if fits else 1, 0], dtype=torch.int32))
            if fits:
                view(p[3], U8, (len(data),)).copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
            return
        if int(rec['kind']) != 36 or flags not in (256, 512):
            return self.inner.run_one(rec)
        P, H, W, plane, ldrow, OH, OW = i[:7]
        # the launcher's alignment rules (csrc/matte.hip): outputs and the layer 16 bytes, planes, ids and the colour table 4
        assert p[0] % 4 == 0 and p[4] % 16 == 0, 'planes (p0) 4-byte, matte plane (p4) 16-byte aligned'
        if flags == 512:
            assert p[2] % 16 == 0, 'output planes (p2) 16-byte aligned'
        else:
            assert p[3] % 16 == 0 and p[7] % 16 == 0 and p[5] % 4 == 0 and p[6] % 4 == 0, 'output frame (p3) and layer (p7) 16-byte, ids (p5) and colours (p6) 4-byte aligned'
        planes = view(p[0], F32, (P, H, W), (plane, ldrow, 1)).numpy() if p[0] else None
        if flags == 512:
            if P > 1:
                view(p[2], U8, (P - 1, OH, OW)).copy_(torch.from_numpy(soft(planes, OH, OW)))
            self.softs += 1
            self.log.append(('soft', soft(planes, OH, OW) if P > 1 else None))
            return
        mode = {v: k for k, v in MODE_CODES.items()}[i[8]]
        targets = list((ctypes.c_int32 * i[9]).from_address(p[1])) if i[9] else []
        frame = view(p[2], U8, (OH, OW, 3), (i[7], 3, 1)).numpy() if p[2] else None
        out, a = composite(mode, frame, planes, targets, ids=view(p[5], U8, (OH, OW)).numpy() if p[5] else None,
                           table=view(p[6], U8, (256, 4)).numpy() if p[6] else None,
                           layer_rgba=view(p[7], U8, (OH, OW, 4)).numpy() if p[7] else None, out_hw=(OH, OW), want_alpha=bool(p[4]))
        if out is not None:
            view(p[3], U8, (OH, OW, 3)).copy_(torch.from_numpy(out))
        if a is not None:
            view(p[4], U8, (OH, OW)).copy_(torch.from_numpy(a))
        self.composites += 1
        self.log.append((mode, out, a, targets))

    def run(self, arr):
        for rec in arr:
            self.run_one(rec)
