"""One saver run shared by the CPU test (through tests/mock_exec_png_photo.py) and the GPU test: three frames of the bike example with
synthetic probability planes through ResultSaver(cutout=True, alpha_matte=True, soft_masks=True, png_codes='dynamic'), and the same
frames with the fixed codes; the files are read back with PIL."""
import os
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
H, W = 120, 214                      # the bike frames, reduced four times


def frames():
    out = []
    for t in range(3):
        im = Image.open(os.path.join(HERE, 'golden', 'bike', f'{t:05d}.jpg')).convert('RGB').resize((W, H))
        out.append(np.array(im))
    return out


def planes(t, P=3, h=60, w=108):
    """soft probability planes at half the output size: two blobs that move with t, as the un-padded view of a padded buffer"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    a = np.exp(-(((yy - 25 - t) / 12) ** 2 + ((xx - 40 - 2 * t) / 18) ** 2))
    b = np.exp(-(((yy - 35) / 9) ** 2 + ((xx - 75 + t) / 11) ** 2))
    logits = np.stack([np.full((h, w), 0.35, np.float32), a, b]) * 6
    e = np.exp(logits - logits.max(0))
    buf = torch.full((P, h + 3, w + 8), 7.0)
    buf[:, 1:1 + h, 2:2 + w] = torch.from_numpy((e / e.sum(0)).astype(np.float32))
    return buf[:, 1:1 + h, 2:2 + w]


def saver(out, device, **kw):
    from cutie_amd.inference.object_manager import ObjectManager
    from cutie_amd.inference.utils.results_utils import ResultSaver
    om = ObjectManager()
    om.add_new_objects([5, 3])

    def to_mask(prob, dtype=torch.int64):
        return torch.tensor([0, 5, 3], device=prob.device)[prob.argmax(0)].to(dtype)
    proc = types.SimpleNamespace(network=types.SimpleNamespace(device=torch.device(device)), object_manager=om, output_prob_to_mask=to_mask)
    return ResultSaver(out, 'vid', dataset='generic', object_manager=om, use_long_id=False, processor=proc, **kw)


def run(out, device, **kw):
    s = saver(out, device, **kw)
    for t, fr in enumerate(frames()):
        s.process(planes(t).to(device), f'{t:05d}.jpg', resize_needed=True, shape=(H, W), image_u8=torch.from_numpy(fr).to(device))
    s.end()
    files = {}
    for dp, _, fs in os.walk(out):
        for f in fs:
            files[os.path.relpath(os.path.join(dp, f), out).replace(os.sep, '/')] = os.path.join(dp, f)
    return files


def run_and_check(tmp, device='cpu', egress='host'):
    dyn = run(os.path.join(tmp, 'dynamic'), device, egress=egress, cutout=True, alpha_matte=True, soft_masks=True, png_codes='dynamic', target_objects=[3])
    fix = run(os.path.join(tmp, 'fixed'), device, egress=egress, alpha_matte=True, soft_masks=True, target_objects=[3])
    assert sorted(set(dyn) - set(fix)) == [f'vid/cutout/{t:05d}.png' for t in range(3)] and set(fix) <= set(dyn)
    assert len(fix) == 3 * (1 + 1 + 2)                                           # per frame the mask, the matte and two soft masks
    smaller = 0
    for t, fr in enumerate(frames()):
        cut = Image.open(dyn[f'vid/cutout/{t:05d}.png'])
        assert cut.mode == 'RGBA' and cut.size == (W, H)
        cut = np.array(cut)
        alpha = Image.open(dyn[f'vid/alpha/{t:05d}.png'])
        assert alpha.mode == 'L'
        assert np.array_equal(cut[..., :3], fr)                                  # RGB is the frame
        assert np.array_equal(cut[..., 3], np.array(alpha))                      # A is the alpha file of the same run
        assert 0 < int(cut[..., 3].max()) and int(cut[..., 3].min()) == 0 and len(np.unique(cut[..., 3])) > 16      # a soft matte of object 3
    for name in fix:                                                             # the dynamic files hold the pixels of the fixed ones
        a, b = Image.open(dyn[name]), Image.open(fix[name])
        assert a.mode == b.mode and np.array_equal(np.array(a), np.array(b)), name
        if '/alpha/' in name or '/soft_masks/' in name:
            smaller += os.path.getsize(dyn[name]) < os.path.getsize(fix[name])
        else:
            assert open(dyn[name], 'rb').read() == open(fix[name], 'rb').read()  # the id masks never change encoder
    assert smaller == 9                                                          # every smooth plane took fewer bytes
    return dyn, fix
