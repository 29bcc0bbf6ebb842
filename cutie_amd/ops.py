"""Launch-plan builder: Python mirror of the ``cutie_op`` descriptor of include/cutie_hip.h.

An ``OpList`` records kernel descriptors over torch-allocated device buffers (torch = memory + stream
plumbing only); ``run()`` hands the whole array to ``cutie_exec`` in ONE C call.  Pointer slots can be
declared *dynamic* (named) and patched per call, so a cached plan is reused across frames.
"""
import os

import numpy as np
import torch

from . import _lib

NI, NF, NP = 24, 6, 16
OP_DTYPE = np.dtype([('kind', '<i4'), ('flags', '<i4'), ('i', '<i4', (NI,)), ('f', '<f4', (NF,)), ('p', '<u8', (NP,))])
assert OP_DTYPE.itemsize == _lib.OP_STRUCT_SIZE

# op kinds (include/cutie_hip.h)
(CONV, MAXPOOL, IMG_PREP, UPSAMPLE2X_ADD, AREA_DOWN, MASK_DOWN, GAP, ECA_APPLY, GRU, SEG_AGG, UP4_SOFTMAX,
 MASK_MERGE, AGG_SOFTMAX, LINEAR, LAYERNORM, QUERY_INIT, AUX_MASK, ATTN_Q2P, ATTN_SELF, ATTN_P2Q, SUMMARIZE,
 ADD_PE, KEY_PREP, AFF_SCORE, AFF_SELECT, AFF_READOUT, MEMSET32, COPY2D, AXPY, USAGE_TICK, RANK_SELECT,
 GATHER_ROWS, CONSOL_AFF, CONSOL_READ, CAST, PROB_TO_ID, RESIZE, FLIP_W, AREA_DOWN3, QFFN, STEM, BANK_WRITE) = range(1, 43)

KIND_NAMES = {}
for _n in ('CONV MAXPOOL IMG_PREP UPSAMPLE2X_ADD AREA_DOWN MASK_DOWN GAP ECA_APPLY GRU SEG_AGG UP4_SOFTMAX MASK_MERGE '
           'AGG_SOFTMAX LINEAR LAYERNORM QUERY_INIT AUX_MASK ATTN_Q2P ATTN_SELF ATTN_P2Q SUMMARIZE ADD_PE KEY_PREP '
           'AFF_SCORE AFF_SELECT AFF_READOUT MEMSET32 COPY2D AXPY USAGE_TICK RANK_SELECT GATHER_ROWS CONSOL_AFF '
           'CONSOL_READ CAST PROB_TO_ID RESIZE FLIP_W AREA_DOWN3 QFFN STEM').split():
    KIND_NAMES[globals()[_n]] = _n

F_RELU_IN, F_OUT_F32, F_RES_BCAST = 1, 2, 4
# launches of the frame's critical path raise their waves' issue priority (include/cutie_hip.h CUTIE_F_PRIO)
F_PRIO, F_AFF_PRIO = 256, 64
F_TILE_OFF = 128 if os.environ.get('CUTIE_AMD_COUT1_TILE', '1') in ('', '0') else 0  # A/B switch of conv_cout1_tile_kernel
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SQ1 = 0, 1, 2, 3
ACT_SHIFT = 4
AREA_RT = 8 if os.environ.get('CUTIE_AMD_AREA_R', '1') in ('', '0') else 0          # AREA_DOWN3 flags&8: bodies with a run-time pooling ratio (A/B switch)
GRU_SCALAR = 1 if os.environ.get('CUTIE_AMD_GRU4', '1') in ('', '0') else 0            # GRU flags&1: one channel per thread (A/B switch)
KEYPREP_LOOP = 2 if os.environ.get('CUTIE_AMD_KEYPREP_LOOP', '0') not in ('', '0') else 0   # KEY_PREP flags&2: c_j by one lane per row (A/B switch)
UP4_LANES = 16 if os.environ.get('CUTIE_AMD_UP4_SHARED', '1') in ('', '0') else 0     # UP4_SOFTMAX flags&16 (mask-down form): every lane aggregates its own six source pixels (A/B switch)
SELECT_COARSE = 2 if os.environ.get('CUTIE_AMD_SELECT_FINE', '1') in ('', '0') else 0    # AFF_SELECT flags&2: 16 | 32 | 64 values per lane only (A/B switch)
UP4_RTK = 8 if os.environ.get('CUTIE_AMD_UP4_KC', '1') in ('', '0') else 0           # UP4_SOFTMAX flags&8: kernels with a run-time object count (A/B switch)

# conv tile table (mirrors the switch in csrc/conv_igemm.hip): id -> (BM, BN, BK)
TILES = {0: (128, 128, 32), 1: (128, 64, 32), 2: (64, 64, 32), 3: (256, 16, 32), 4: (64, 128, 32),
         5: (64, 64, 64), 6: (64, 128, 64), 7: (128, 128, 64), 8: (64, 64, 128), 9: (32, 64, 64),
         10: (128, 64, 64), 11: (32, 64, 128), 12: (32, 128, 64),
         13: (64, 64, 64), 14: (128, 64, 64), 15: (64, 128, 64), 16: (128, 128, 64), 17: (64, 64, 128), 18: (128, 128, 32),   # 13+: 8 waves
         # 20+: WK K groups per block (intra-block split-K: WK copies of the 4-wave pipeline on one output tile)
         20: (64, 64, 64), 21: (64, 64, 128), 22: (32, 64, 128), 23: (128, 64, 64), 24: (64, 128, 64), 25: (128, 128, 64),
         26: (32, 64, 64), 27: (64, 64, 64), 28: (32, 64, 64), 29: (64, 128, 32), 30: (64, 64, 32)}
TILE_WK = {20: 2, 21: 2, 22: 2, 23: 2, 24: 2, 25: 2, 26: 2, 27: 4, 28: 4, 29: 2, 30: 2}
# (Round 3 removed three kernel families that no geometry of the cold-cache sweeps selects any more -- profiles/r03_conv_sweep_cold.md:
# 40..44 patch-resident 3x3 in the register-staged kernel, 50..56 buffer-load kernel, 90..95 strip-resident 3x3.  The halo tiles of
# conv_pc.hip, 120.., are what became of the resident-input idea.)

# 60+: LDS-DMA kernel (conv_dma.hip): operands global -> LDS by buffer_load ... lds, rolled K loop with ~2-4 non-MFMA
# instructions per MFMA.  id -> (BM, BN, BK); needs Cin % 64 == 0 (both sources of a virtual concat), no split-K.
DMA_TILES = {60: (128, 128, 64), 61: (128, 128, 64), 62: (128, 128, 64), 63: (128, 64, 64), 64: (64, 128, 64), 65: (64, 64, 64),
             66: (64, 64, 64), 67: (32, 64, 64), 68: (256, 128, 64), 69: (32, 128, 64), 70: (128, 128, 64), 71: (128, 64, 64),
             72: (64, 64, 64), 73: (64, 64, 64), 74: (64, 64, 64), 75: (32, 64, 64), 76: (128, 64, 64), 77: (64, 128, 64), 78: (32, 128, 64),
             80: (64, 64, 128), 81: (64, 64, 128), 82: (32, 64, 128), 83: (32, 64, 128), 84: (64, 128, 128), 85: (128, 64, 128),
             86: (96, 64, 64), 87: (96, 64, 64), 88: (64, 64, 64), 89: (64, 64, 64)}


# 100+: conv_pc.hip -- producer / consumer split (NPW producer waves issue every LDS-DMA piece, WM x WN consumer waves only read
# fragments and issue MFMAs), epilogue straight from the accumulators.  100..: stream mode (any kernel size / stride);
# 120..: halo mode, 3x3 / stride 1 / pad 1 with the (TH+2) x (TW+2) input patch of a 64-channel slice resident in LDS.
# id -> (BM, BN, BK); PC_HALO: id -> (TH, TW)
PC_TILES = {100: (64, 64, 64), 101: (64, 64, 64), 102: (32, 64, 64), 103: (128, 64, 64), 104: (64, 128, 64), 105: (128, 128, 64),
            106: (128, 128, 64), 107: (64, 64, 64), 108: (128, 128, 64), 109: (32, 64, 64), 110: (96, 64, 64), 111: (96, 128, 64),
            120: (64, 64, 64), 121: (64, 64, 64), 122: (128, 64, 64), 123: (128, 128, 64), 124: (64, 128, 64), 125: (32, 64, 64),
            126: (128, 128, 64), 127: (64, 128, 64), 129: (96, 64, 64), 130: (32, 64, 64), 131: (64, 128, 64),
            132: (64, 64, 64), 133: (96, 128, 64), 134: (320, 64, 64),
            # pair steps (two K tiles per barrier): UNMEASURED, branch next/pc-pairstep
            140: (64, 64, 64), 141: (96, 64, 64), 142: (96, 64, 64), 143: (32, 64, 64), 144: (128, 64, 64),
            145: (96, 64, 64), 146: (128, 64, 64), 147: (32, 64, 64)}
PC_HALO = {120: (8, 8), 121: (4, 16), 122: (8, 16), 123: (8, 16), 124: (8, 8), 125: (4, 8), 126: (8, 16), 127: (4, 16),
           129: (10, 9), 130: (5, 6), 131: (6, 9), 132: (6, 9), 133: (10, 9), 134: (20, 16),
           145: (10, 9), 146: (8, 16), 147: (5, 6)}

ALL_TILES = {**TILES, **DMA_TILES, **PC_TILES}


def korder_class(tile, splitk=1):
    """Which fp32 summation order over K a conv tile implements -- two tiles of one class give bit-identical outputs on the same
    operands (tests/test_gpu_kernels.py::test_tiles_of_a_korder_class_agree_bitwise).  'stream': K tiles in the packed order
    k = (kh * KW + kw) * Cin + c, two v_mfma_f32_16x16x32_bf16 per 64 channels in ascending k (conv_dma.hip, the stream tiles of
    conv_pc.hip); 'igemm': the register-staged tiles without split-K (same order, not asserted against 'stream'); 'halo': 64-channel slice outermost, its nine taps inside
    (conv_pc.hip, tiles 120..); anything that splits K (WK tiles, split-K) is a class of its own."""
    if tile in PC_HALO:
        return 'halo'
    if tile in TILE_WK or splitk != 1:
        return ('split', tile, splitk)
    if tile in (3, COUT1_TILE):
        return ('small', tile)
    return 'stream' if (tile in DMA_TILES or tile in PC_TILES) else 'igemm'


def pc_tile_ok(tile, *, cin, kh, stride=1, pad=None, c2=0):
    """conv_pc_kernel eligibility (mirrors launch_pc in conv_pc.hip)."""
    if cin % 64 or (c2 and (c2 % 64 or (cin - c2) % 64)) or kh > 5:
        return False
    if tile in PC_HALO:
        return kh == 3 and stride == 1 and (pad is None or pad == 1)
    return True


def pc_blocks(tile, B, OH, OW, cout):
    """Workgroups of a conv on a conv_pc tile."""
    bm, bn, _ = PC_TILES[tile]
    if tile in PC_HALO:
        th, tw = PC_HALO[tile]
        return B * -(-OH // th) * -(-OW // tw) * -(-cout // bn)
    return -(-(B * OH * OW) // bm) * -(-cout // bn)


def dma_tiles_enabled():
    return os.environ.get('CUTIE_AMD_DMA_TILES', '1') not in ('', '0')


def dma_tile_ok(tile, *, cin, kh, c2=0):
    """conv_dma_kernel eligibility (mirrors launch_dma in conv_dma.hip): a K tile (64 or 128 channels) never straddles a tap or a
    source."""
    bk = DMA_TILES[tile][2]
    return cin % bk == 0 and (c2 == 0 or (c2 % bk == 0 and (cin - c2) % bk == 0)) and kh * kh <= 32


def conv_side_jobs_ok(*, cin, cout, kh, c2=0):
    """Can a conv of this geometry carry the GAP accumulation / zero job (conv_dma_kernel only)?"""
    return dma_tiles_enabled() and dma_tile_ok(60, cin=cin, kh=kh, c2=c2) and cout % 8 == 0 and cout > 16


NUM_CU = 256
# bytes of the next conv's weights a conv_pc launch touches on its way out (0: off); CUTIE_AMD_WPF overrides
WEIGHT_PREFETCH = int(os.environ.get('CUTIE_AMD_WPF', str(8 << 20)))
WEIGHT_PREFETCH_BLOCK = int(os.environ.get('CUTIE_AMD_WPF_BLOCK', str(48 << 10)))      # bytes per block (see OpList.finalize)


COUT1_TILE = 19          # dedicated per-pixel dot-product kernel (conv_cout1_kernel)


def cout1_ok(cout, cin, c2=0, res=False):
    lp = cin // 8
    return cout == 1 and c2 == 0 and not res and cin % 8 == 0 and 1 <= lp <= 64 and (lp & (lp - 1)) == 0


def tile_candidates(M, cout, cin, kpad=None, geom=None):
    """Tile ids that are legal for a conv (BK > 32 needs Cin >= 32; tiny Cout uses the 256x16 tile; the K groups of a
    WK tile must divide the K tiles; geom = dict(kh, stride, pad, W, c2) enables the LDS-DMA families)."""
    if cout <= 16:
        return [3] + ([COUT1_TILE] if cout1_ok(cout, cin) else [])
    out = []
    for t, (bm, bn, bk) in TILES.items():
        if t == 3 or (bk > 32 and cin < 32):
            continue
        wk = TILE_WK.get(t, 1)
        if wk > 1 and (kpad is None or (kpad // bk) % wk or kpad // bk < 2 * wk):
            continue
        if bn == 128 and cout <= 64:
            continue
        if bm * 2 > max(M, 64) * 2 and bm > 64:          # do not pad a tiny M to a huge tile
            continue
        out.append(t)
    if dma_tiles_enabled() and geom is not None and dma_tile_ok(60, cin=cin, kh=geom['kh'], c2=geom.get('c2', 0)):
        for t, (bm, bn, bk) in DMA_TILES.items():
            if not (bn == 128 and cout <= 64) and not (bm > 64 and bm > max(M, 64)) and not (bm == 256 and M < 16384) \
                    and dma_tile_ok(t, cin=cin, kh=geom['kh'], c2=geom.get('c2', 0)):
                out.append(t)
    if dma_tiles_enabled() and geom is not None:
        for t, (bm, bn, bk) in PC_TILES.items():
            if pc_tile_ok(t, cin=cin, kh=geom['kh'], stride=geom.get('stride', 1), pad=geom.get('pad'), c2=geom.get('c2', 0)) \
                    and not (bn == 128 and cout <= 64) and not (bm > 64 and bm > max(M, 64)) and not (bm == 256 and M < 16384):
                out.append(t)
    return out


SPLITK_PART_FLOATS = 16 << 20           # 64 MiB of fp32 partial tiles
_splitk_scratch = {}


def splitk_scratch(device, owner=None):
    """fp32 partial-tile scratch of split-K convs.  One buffer per owner (an Engine: the launches of one engine are
    stream-ordered, engines forked for concurrent clips must not share partials; it lives and dies with the owner);
    owner None = one per device."""
    dev = torch.device(device)
    store = _splitk_scratch if owner is None else owner.__dict__.setdefault('_splitk_part', {})
    key = str(dev)
    if key not in store:
        n = SPLITK_PART_FLOATS if dev.type == 'cuda' else 1024
        store[key] = torch.zeros(n, dtype=torch.float32, device=device)
    return store[key]


def splitk_candidates(M, cout, kpad, tile):
    """Split-K factors worth timing for a conv on a given tile: only when the plain grid leaves CUs idle."""
    if tile == COUT1_TILE or tile == 3 or tile in DMA_TILES or tile in PC_TILES:
        return [1]
    bm, bn, bk = TILES[tile]
    blocks = -(-M // bm) * -(-cout // bn)
    nk = kpad // bk // TILE_WK.get(tile, 1)
    ldp = (cout + 7) & ~7
    out = [1]
    for sk in (2, 3, 4, 6, 8, 9, 12, 16, 18):
        if blocks >= NUM_CU or blocks * sk > 6 * NUM_CU or nk // sk < 2:
            break
        if sk * M * ldp > SPLITK_PART_FLOATS:
            break
        if nk % sk == 0:                                 # equal slices only (conv_igemm.hip)
            out.append(sk)
    return out


def pick_tile(M, cout, cin=64, geom=None):
    """Static, deterministic tile choice for conv geometries that are not in the tuned table (cutie_amd/tiles_gfx950.json):
    the largest tile that still yields >= NUM_CU workgroups, else the one with the most workgroups -- among the LDS-DMA tiles
    when the conv is eligible for them (geom = dict(kh, c2) given and Cin % 64 == 0), else among the register-staged ones."""
    if cout <= 16:
        return 3
    if geom is not None and dma_tiles_enabled() and dma_tile_ok(60, cin=cin, kh=geom['kh'], c2=geom.get('c2', 0)):
        # order fitted on the cold-cache sweeps of the 480p (K = 1, 2, 3) and 1080p (K = 5) geometries (producer / consumer tiles)
        cands = [t for t in (108, 103, 110, 101, 102) if pc_tile_ok(t, cin=cin, kh=geom['kh'], c2=geom.get('c2', 0))]
    else:
        cands = [6, 5, 9] if cin >= 32 else [4, 2]
    if cout <= 64:
        cands = [c for c in cands if ALL_TILES[c][1] <= 64] or [2]
    best, best_blocks = None, -1
    for t in cands:
        bm, bn, _ = ALL_TILES[t]
        blocks = -(-M // bm) * -(-cout // bn)
        if blocks >= NUM_CU:
            return t
        if blocks > best_blocks:
            best, best_blocks = t, blocks
    return best


def static_tile(M, cout, cin, kh, c2=0, res=False, side=False, cout1=None):
    """The tile a conv takes when the tile table has no entry for it: the Cout = 1 kernel where it applies (never with a residual, a second
    source or a side job), else pick_tile.  ONE statement of the rule for OpList.conv, for the K-order twins of Plan.autotune_convs and for
    the cuts of a mixed lock-step plan (Plan.conv): a clip's bits follow from the tile its one-clip plan takes.  cout1 (a finished descriptor,
    whose operands are no longer at hand): was the launch given the Cout = 1 kernel -- that part of the rule does not look at M."""
    if (cout1_ok(cout, cin, c2, res) and not side) if cout1 is None else cout1:
        return COUT1_TILE
    return pick_tile(M, cout, cin, dict(kh=kh, c2=c2))


def conv_tile_key(M, cout, cin, kh, stride, relu_in, out_f32, H, W):
    """Key of a conv geometry in the tile table (cutie_amd/tiles_gfx950.json, Engine.tile_cache): M = B x OH x OW rows, H x W the input."""
    return (int(M), int(cout), int(cin), int(kh), int(stride), (1 if relu_in else 0) | (2 if out_f32 else 0), int(H), int(W))


def aa_taps(n_in, n_out):
    """Tap ranges and weights of F.interpolate(mode='bilinear', align_corners=False, antialias=True) along one axis, rounded as
    torch's CPU kernel rounds them (aten/src/ATen/native/cpu/UpSampleKernel.cpp, _compute_weights_aa for float input): scale and
    support in fp32, center = fp32(scale * (i + 0.5)), the tap bounds truncate fp32(center -+ support) + 0.5 evaluated in fp64,
    each weight is filter(fp32((fp32(j - center) + 0.5) * invscale)) with the fp64 product, the sum and the normalisation in fp32.
    An axis whose size does not change is the identity (torch skips that pass).  -> (first int64 [n_out], count int64 [n_out],
    weights f32 [n_out, K])."""
    f32 = np.float32
    i = np.arange(n_out)
    if n_in == n_out:
        return i, np.ones(n_out, dtype=np.int64), np.ones((n_out, 1), dtype=f32)
    scale = f32(n_in) / f32(n_out)
    support = scale if scale >= 1 else f32(1.0)
    invscale = f32(1.0 / np.float64(scale)) if scale >= 1 else f32(1.0)
    max_taps = int(np.ceil(support)) * 2 + 1
    center = (np.float64(scale) * (i + 0.5)).astype(f32)
    first = np.maximum(((center - support).astype(np.float64) + 0.5).astype(np.int64), 0)
    count = np.minimum(((center + support).astype(np.float64) + 0.5).astype(np.int64), n_in) - first
    count = np.clip(count, 0, max_taps)
    j = np.arange(max_taps)
    pos = (first[:, None] + j[None, :]).astype(f32)
    arg = (((pos - center[:, None]).astype(np.float64) + 0.5) * np.float64(invscale)).astype(f32)
    arg = np.abs(arg)
    w = np.where(arg < 1, f32(1.0) - arg, f32(0.0)).astype(f32)
    w[j[None, :] >= count[:, None]] = 0
    total = np.zeros(n_out, dtype=f32)
    for k in range(max_taps):                                   # fp32, ascending taps
        total = (total + w[:, k]).astype(f32)
    nz = total != 0
    w[nz] = (w[nz] / total[nz, None]).astype(f32)
    return first, count, w


def resize_aa_table(H, W, OH, OW):
    """The tap table of an antialiased RESIZE (p2): int32 [OW + OH, K + 2], row = (first tap, tap count, K fp32 weights as bits);
    rows 0..OW-1 the horizontal pass, then OH rows of the vertical pass."""
    parts = [aa_taps(W, OW), aa_taps(H, OH)]
    K = max(int(w.shape[1]) for _, _, w in parts)
    tab = np.zeros((OW + OH, K + 2), dtype=np.int32)
    r = 0
    for first, count, w in parts:
        n = len(first)
        tab[r:r + n, 0], tab[r:r + n, 1] = first, count
        tab[r:r + n, 2:2 + w.shape[1]] = w.view(np.int32)
        r += n
    return tab


def pack_counts(counts):
    """The object counts of the clips of a lock-step group as ONE word of 3-bit fields, clip c at bits 3c .. 3c + 2 (include/cutie_hip.h, "mixed
    forms"): at most 8 clips of 1 .. 7 objects; a zero field ends the list."""
    counts = [int(k) for k in counts]
    assert 1 <= len(counts) <= 8 and all(1 <= k <= 7 for k in counts), counts
    return sum(k << (3 * c) for c, k in enumerate(counts))


def clip_starts(counts):
    """Prefix sums of the counts: clip c holds the objects [starts[c], starts[c + 1])."""
    st = [0]
    for k in counts:
        st.append(st[-1] + int(k))
    return st


class Dyn:
    """A named, per-call patched pointer (optionally with a byte offset)."""
    __slots__ = ('name', 'offset')

    def __init__(self, name, offset=0):
        self.name, self.offset = name, offset


def _ptr(t):
    if t is None:
        return 0
    if isinstance(t, int):
        return t
    return t.data_ptr()


def _need_form(has, words):
    """A form that came without a new ABI number: a library built before it (``has``: its _lib.has_* probe) is named as stale, in
    ``words``.  (An injected interpreter of the tests has no library; a missing library fails when the list runs.)"""
    try:
        known = getattr(_lib._executor, 'is_mock', False) or has()
    except _lib.HipLibraryError:
        known = True
    if not known:
        raise _lib.HipLibraryError(f'{_lib.LIB_PATH} is stale ({words}); rebuild it.')


def _u8_plane(who, name, t, hw=None):
    """``t`` is a contiguous uint8 [H, W] -- of the size ``hw`` when given -- with H, W >= 1 and H * W < 2^31.  -> (H, W)"""
    shaped = t.dim() == 2 if hw is None else tuple(t.shape) == tuple(hw)
    if t.dtype != torch.uint8 or not shaped or not t.is_contiguous():
        if hw is None or (min(hw) >= 1 and hw[0] * hw[1] < 1 << 31):        # (a size given apart is judged first)
            raise ValueError(f"{who}: {name} is a contiguous uint8 {'[H, W]' if hw is None else list(hw)}, not {t.dtype} {tuple(t.shape)}")
    H, W = hw if hw is not None else (int(t.shape[0]), int(t.shape[1]))
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise ValueError(f'{who}: a plane of {H} x {W}: H, W >= 1 and H * W < 2^31')
    return H, W


def _object_ids(who, name, objects):
    """Object ids as a sequence of ints or as an int32 tensor of them on the device, which is not inspected.
    -> (n, the tensor or None, the list or None)"""
    if torch.is_tensor(objects):
        if objects.dtype != torch.int32 or objects.dim() != 1 or not objects.is_contiguous():
            raise ValueError(f'{who}: {name} on the device are a contiguous int32 [n]')
        return int(objects.numel()), objects, None
    listed = [int(v) for v in objects]
    return len(listed), None, listed


JPEG_SYNC_ROUNDS = 4        # sync rounds of the speculative Huffman decode before a segment is finished serially (jpeg.hip)


class OpList:
    # kinds whose kernels raise their waves' issue priority under F_PRIO (include/cutie_hip.h); CONV and the affinity ops carry a `prio` argument
    PRIO_KINDS = frozenset((UPSAMPLE2X_ADD, AREA_DOWN3, ECA_APPLY, GRU, UP4_SOFTMAX, ATTN_Q2P, ATTN_SELF, ATTN_P2Q, QFFN))

    def __init__(self, scratch_owner=None, touch_next_weights=True, prio=True):
        self.prio = prio                     # the launches of this list belong to the frame's critical path (plans.Plan.prio)
        self.scratch_owner = scratch_owner   # see splitk_scratch
        self.touch_next_weights = touch_next_weights   # see finalize (plans switch it off where weights stay warm between two uses)
        self.recs = []          # (kind, flags, ints, floats, ptrs)
        self.keep = []          # tensors kept alive
        self.wbytes = {}        # conv op index -> bytes of its packed weights
        self.dyn = {}           # name -> [(op index, slot, offset)]
        self.arr = None
        self._words = None      # bind's view of `dyn` and `arr` (rebuilt with the array)

    # ---- generic ------------------------------------------------------------------
    def add(self, kind, flags=0, ints=(), floats=(), ptrs=()):
        idx = len(self.recs)
        if kind in self.PRIO_KINDS and self.prio:
            flags |= F_PRIO
        pl = []
        for slot, t in enumerate(ptrs):
            if isinstance(t, Dyn):
                self.dyn.setdefault(t.name, []).append((idx, slot, t.offset))
                pl.append(0)
            else:
                if isinstance(t, torch.Tensor):
                    self.keep.append(t)
                pl.append(_ptr(t))
        self.recs.append((kind, flags, [int(v) for v in ints], [float(v) for v in floats], pl))
        self.arr = self._words = None
        return idx

    def finalize(self):
        arr = np.zeros(len(self.recs), dtype=OP_DTYPE)
        for n, (kind, flags, ints, floats, ptrs) in enumerate(self.recs):
            arr['kind'][n] = kind
            arr['flags'][n] = flags
            arr['i'][n, :len(ints)] = ints
            arr['f'][n, :len(floats)] = floats
            arr['p'][n, :len(ptrs)] = ptrs
        self.arr = arr
        self._words = None
        self.wire_next_weights()
        return arr

    def wire_next_weights(self):
        """CONV p9 / i22, p10 / i23 of the finalized array, from the tiles it carries NOW (plans call this again once the tile table
        has been applied): a producer / consumer conv touches the packed weights of the conv behind it in the list when its own DMA
        is out, and those of the conv after that one when the next conv has no producer waves (conv_pc.hip)."""
        arr = self.arr
        convs = [n for n in range(len(arr)) if arr['kind'][n] == CONV]
        for n in convs:
            arr['p'][n, 9:11] = 0
            arr['i'][n, 22:24] = 0
        if not (WEIGHT_PREFETCH and self.touch_next_weights):
            return
        nxt, nxt2 = None, None                               # (weights, bytes, has producer waves) of the next conv / of the one after it
        for n in reversed(convs):
            i = arr['i'][n]
            pc = int(i[17]) in PC_TILES
            if nxt is not None and pc:
                # the blocks of one XCD share the range: a block that pulls much more than ~48 KB through its CU outlasts the
                # consumers' epilogue (bytes per CU), so small grids touch only the head of large weights
                budget = WEIGHT_PREFETCH_BLOCK * -(-pc_blocks(int(i[17]), int(i[0]), int(i[7]), int(i[8]), int(i[9])) // 8)
                n1 = min(nxt[1], WEIGHT_PREFETCH, budget)
                arr['p'][n, 9], arr['i'][n, 22] = nxt[0], n1
                n2 = min(nxt2[1], WEIGHT_PREFETCH, budget - n1) if (nxt2 is not None and not nxt[2]) else 0
                if n2 > 0:                                   # the next conv cannot do it for its successor
                    arr['p'][n, 10], arr['i'][n, 23] = nxt2[0], n2
            nxt, nxt2 = (int(arr['p'][n, 2]), self.wbytes[n], pc), nxt

    def patch_ints(self, op, start, values):
        """Overwrite ints [start, start + len(values)) of record `op` -- in the recorded list and, when the array exists, in place (a
        plan whose launches stay the same while a few sizes change: the affinity plans of a bucket between two memory frames)."""
        values = [int(v) for v in values]
        ints = self.recs[op][2]
        end = start + len(values)
        if len(ints) < end:
            ints.extend([0] * (end - len(ints)))
        ints[start:end] = values
        if self.arr is not None:
            self.arr['i'][op, start:end] = values

    def bind(self, **tensors):
        """Patch dynamic pointer slots.  Values: torch tensors or raw ints.  (Host time: this runs five times per frame with a dozen
        names each -- the slots of a name are 64-bit word indices into the descriptor array, written through one memoryview.)"""
        if self.arr is None:
            self.finalize()
        words = self._words
        if words is None:
            # a descriptor is 32 words; its pointer field starts at word 16 (include/cutie_hip.h, asserted against the dtype)
            assert OP_DTYPE.itemsize == 256 and OP_DTYPE.fields['p'][1] == 128
            words = self._words = ({name: tuple((idx * 32 + 16 + slot, off) for (idx, slot, off) in sl) for name, sl in self.dyn.items()},
                                   memoryview(self.arr).cast('B').cast('Q'))
        table, mv = words
        for name, t in tensors.items():
            sl = table.get(name)
            if sl is None:
                continue
            base = 0 if t is None else (t if type(t) is int else t.data_ptr())
            if base:
                for w, off in sl:
                    mv[w] = base + off
            else:
                for w, off in sl:
                    mv[w] = 0

    def run(self, _stream=None, **tensors):
        """_stream: a torch stream other than the current one to launch on (the executor is handed its raw handle; an executor
        without `run_on` -- the recording shims, the interpreter of the tests -- runs inside torch's stream context instead)."""
        if self.arr is None:
            self.finalize()
        if tensors:
            self.bind(**tensors)
        ex = _lib.get_executor()
        if _stream is None:
            ex.run(self.arr)
        elif hasattr(ex, 'run_on'):
            ex.run_on(self.arr, _stream)
        else:
            with torch.cuda.stream(_stream):
                ex.run(self.arr)

    def __len__(self):
        return len(self.recs)

    # ---- builders (argument order mirrors include/cutie_hip.h) -----------------------
    def conv(self, x1, w, y, *, B, H, W, C1, ldx1, OH, OW, ldy, stride=1, pad=0, x2=None, C2=0, ldx2=0,
             res=None, ldr=0, res_bcast=False, relu_in=False, act=ACT_NONE, out_f32=False, tile=None, splitk=1,
             gap_acc=None, zero=None, prio=False, res_group=None):
        """w: PackedConv (weights.py).  res_group = (objects per clip, rows between the clips' residual maps) with res_bcast: clips in lock step
        (include/cutie_hip.h CONV, ABI 4) -- the B objects come in groups, every group adds its own broadcast residual.  gap_acc: int64 [B, Cout] -- the conv adds the per-(object, channel) sums of its stored output
        (fixed point x 2^24) to it (ECA's global average pool without a launch of its own); zero: an int64 tensor cleared by this
        launch (the accumulator of the NEXT conv).  Both need an LDS-DMA tile (the tile choice is restricted accordingly)."""
        flags = (F_RELU_IN if relu_in else 0) | (F_OUT_F32 if out_f32 else 0) | (F_RES_BCAST if res_bcast else 0) | (act << ACT_SHIFT) | F_TILE_OFF | \
            (F_PRIO if prio else 0)
        assert C1 + C2 == w.cin_padded, (C1, C2, w.cin_padded)
        M = B * OH * OW
        side = gap_acc is not None or zero is not None
        if tile is None:
            tile = static_tile(M, w.cout, C1 + C2, w.kh, C2, res is not None, side)
        if side:
            assert (tile in DMA_TILES or tile in PC_TILES) and not out_f32 and w.cout % 8 == 0 and ldy % 8 == 0, 'GAP accumulation needs an LDS-DMA conv (see conv_side_jobs_ok)'
        part = splitk_scratch(w.weight.device, self.scratch_owner)
        self.wbytes[len(self.recs)] = w.weight.numel() * w.weight.element_size()
        return self.add(CONV, flags,
                        [B, H, W, C1, C2, ldx1, ldx2, OH, OW, w.cout, ldy, w.kh, w.kw, stride, pad, ldr, w.kpad, tile, w.cin_real,
                         splitk, part.numel() // 1024, 0 if zero is None else zero.numel()],
                        self._res_group(res_group, res_bcast, B, OH * OW), [x1, x2, w.weight, w.bias, res, y, part, gap_acc, zero])

    @staticmethod
    def _res_group(res_group, res_bcast, B, OHW):
        if res_group is None:
            return []
        kg, stride = int(res_group[0]), int(res_group[1])
        assert res_bcast and kg > 0 and B % kg == 0 and stride >= OHW and stride < (1 << 24), (res_group, B, OHW)
        return [float(kg), float(stride)]

    def maxpool(self, x, y, *, B, H, W, C, relu=False):
        OH, OW = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        return self.add(MAXPOOL, 1 if relu else 0, [B, H, W, C, OH, OW], [], [x, y])

    STEM_MAX_IMAGES = 12

    def stem(self, image, masks, w, y, *, h0, w0, H, W, pad_left, pad_top, K, mean, std, relu=True, more_images=(), mask_stride=0, counts=None):
        """IMG_PREP + 7x7 / stride-2 conv (w: PackedConv, Cin padded to 8, Cout 64) + 3x3 / stride-2 max pool (+ ReLU) in one launch.
        more_images (ABI 4, <= 11): further frames of the SAME launch -- frame f reads more_images[f - 1], the masks `mask_stride` floats
        behind frame f - 1's, and writes behind frame f - 1's output (y holds all frames).
        counts (the mixed form): the frames are clips with THESE object counts -- clip c's masks are the planes (start_c + c) .. of `masks`
        (the probability tensor of a mixed group, from its first object plane on), its output the objects start_c ..; K and mask_stride unused."""
        assert w.cout == 64 and w.kh == 7 and w.cin_padded == 8 and H % 16 == 0 and W % 16 == 0
        more = list(more_images)
        assert len(more) < self.STEM_MAX_IMAGES
        if counts is not None:
            assert len(counts) == 1 + len(more) and len(counts) > 1
            ints = [h0, w0, H, W, pad_left, pad_top, max(counts), w.kpad, len(counts), 0, pack_counts(counts)]
            return self.add(STEM, 1 if relu else 0, ints, list(mean) + list(std), [image, masks, w.weight, w.bias, y] + more)
        ints = [h0, w0, H, W, pad_left, pad_top, K, w.kpad] + ([1 + len(more), int(mask_stride)] if more else [])
        return self.add(STEM, 1 if relu else 0, ints, list(mean) + list(std), [image, masks, w.weight, w.bias, y] + more)

    def img_prep(self, image, masks, y, *, h0, w0, H, W, pad_left, pad_top, K, mean, std):
        return self.add(IMG_PREP, 0, [h0, w0, H, W, pad_left, pad_top, K], list(mean) + list(std), [image, masks, y])

    def upsample2x_add(self, g, skip, y, *, B, h, w, C, skip_group=None):
        """skip_group = (objects per clip, pixels between the clips' skip maps): clips in lock step (ABI 4); objects per clip a sequence: the
        clips' own counts (the mixed form, i6)."""
        ints = [B, h, w, C]
        if skip_group is not None and not isinstance(skip_group[0], int):
            counts, stride = skip_group
            assert sum(counts) == B and stride >= 4 * h * w
            ints += [0, int(stride), pack_counts(counts)]
        elif skip_group is not None:
            kg, stride = int(skip_group[0]), int(skip_group[1])
            assert kg > 0 and B % kg == 0 and stride >= 4 * h * w
            ints += [kg, stride]
        return self.add(UPSAMPLE2X_ADD, 0, ints, [], [g, skip, y])

    def area_down(self, x, y, *, B, H, W, C, ldx, ldy, r, f32_in=False, Cz=None):
        return self.add(AREA_DOWN, 1 if f32_in else 0, [B, H, W, C, ldx, ldy, r, C if Cz is None else Cz], [], [x, y])

    def area_down3(self, segs):
        """Three area poolings in one launch; segs = 3 x dict(x, y, B, H, W, C, ldx, ldy, r, f32_in=False, Cz=None)."""
        assert len(segs) == 3
        ints, ptrs, flags = [], [], 0
        for q, g in enumerate(segs):
            ints += [g['B'], g['H'], g['W'], g['C'], g['ldx'], g['ldy'], g['r'], g['C'] if g.get('Cz') is None else g['Cz']]
            ptrs += [g['x'], g['y']]
            flags |= (1 << q) if g.get('f32_in') else 0
        return self.add(AREA_DOWN3, flags | AREA_RT, ints, [], ptrs)

    def mask_down(self, masks, pair, m16, *, K, H, W, r=16, pair_channels=8):
        """pair_channels: channel pitch of `pair` (8, or 64 when it is the second source of an LDS-DMA conv: channels 8.. are not written)."""
        assert pair_channels % 8 == 0
        return self.add(MASK_DOWN, 0, [K, H, W, r, pair_channels], [], [masks, pair, m16])

    def gap(self, x, y, *, B, HW, C, scratch=None, partial_only=False):
        if scratch is None:
            scratch = torch.zeros((B, -(-HW // 64), C), dtype=torch.float32, device=y.device)
        self._last_gap_scratch = scratch
        return self.add(GAP, 1 if partial_only else 0, [B, HW, C], [], [x, y, scratch])

    def eca_apply(self, x, gap, wk, r, y, *, B, HW, C, part=None, fixed_sums=None, head=None):
        """part: the GAP partials of the preceding gap(..., partial_only=True) (defaults to the last gap scratch);
        fixed_sums: int64 [B, C] sums accumulated by the producing conv (conv(gap_acc=...)) instead.
        head = (PackedConv w of a Cout = 1, 1x1 conv, out f32 [B, HW]): relu(y) . w + bias computed by the same launch (C = 256)."""
        tail = []
        if head is not None:
            w, out = head
            assert C == 256 and w.cout == 1 and w.kh == 1 and w.cin_padded == 256
            tail = [w.weight, w.bias, out]
        if fixed_sums is not None:
            return self.add(ECA_APPLY, 1, [B, HW, C], [], [x, gap, wk, r, y, fixed_sums] + tail)
        if part is None:
            part = self._last_gap_scratch
        return self.add(ECA_APPLY, 0, [B, HW, C], [], [x, gap, wk, r, y, part] + tail)

    def gru(self, values, h, hb, *, n, C):
        return self.add(GRU, GRU_SCALAR, [n, C], [], [values, h, hb])

    def seg_agg(self, logits, agg, *, K, hw):
        return self.add(SEG_AGG, 0, [K, hw], [], [logits, agg])

    def up4_softmax(self, agg, prob, logits_up, *, P, h, w, from_logits=False, mask_down=None, clips=1):
        """from_logits: `agg` holds the K = P - 1 raw logit planes and the aggregation (SEG_AGG) runs inside the launch (P <= 16).
        mask_down = (m16 f32 [K, hw16], pair bf16 [K, h16, w16, pitch], pitch): the launch also writes MASK_DOWN(prob[1:], r = 16).
        clips > 1 (clips in lock step, ABI 4; the four-pixel forms): every array holds that many clips, P planes out / P - 1 in each.
        clips a sequence (the mixed form, i5): the clips' own object counts -- clip c has K_c logit planes in, K_c + 1 planes out, behind those
        of the clips in front; P is ignored (the largest count + 1 is recorded)."""
        if not isinstance(clips, int):
            counts = [int(k) for k in clips]
            assert from_logits and len(counts) > 1 and h % 4 == 0 and w % 4 == 0 and not UP4_RTK, 'the mixed form: compile-time object counts'
            ints = [max(counts) + 1, h, w, 0, len(counts), pack_counts(counts)]
            if mask_down is not None:
                m16, pair, ints[3] = mask_down
                return self.add(UP4_SOFTMAX, 1 | 4 | UP4_LANES, ints, [], [agg, prob, logits_up, m16, pair])
            return self.add(UP4_SOFTMAX, 1, ints, [], [agg, prob, logits_up])
        if mask_down is not None:
            assert from_logits and P <= 8 and h % 4 == 0 and w % 4 == 0
            m16, pair, pitch = mask_down
            return self.add(UP4_SOFTMAX, 1 | 4 | UP4_RTK | UP4_LANES, [P, h, w, pitch, clips], [], [agg, prob, logits_up, m16, pair])
        assert clips == 1 or (from_logits and P <= 8)
        return self.add(UP4_SOFTMAX, (1 | UP4_RTK) if from_logits else 0, [P, h, w, 0, clips], [], [agg, prob, logits_up])

    def mask_merge(self, inmask, pred, src, planes, *, h0, w0, H, W, pad_left, pad_top, Knew, Kold, nfloat, float_mode):
        return self.add(MASK_MERGE, 1 if float_mode else 0, [h0, w0, H, W, pad_left, pad_top, Knew, Kold, nfloat], [],
                        [inmask, pred, src, planes])

    def agg_softmax(self, planes, prob, *, K, HW):
        return self.add(AGG_SOFTMAX, 0, [K, HW], [], [planes, prob])

    def linear(self, x, w, y, *, M, ldx=None, ldy=None, x_add=None, add_rows=0, res=None, relu=False, add_cols=0,
               ln=None, ln_out=None, eps=1e-5):
        """w: PackedLinear.  ln = (gamma, beta): nn.LayerNorm fused in front (ln_out: where to keep the normalised rows);
        add_cols: x_add feeds only the first add_cols output columns."""
        flags = (1 if relu else 0) | (2 if ln is not None else 0)
        return self.add(LINEAR, flags,
                        [M, w.n, w.kd, w.kd if ldx is None else ldx, w.n if ldy is None else ldy, add_rows, add_cols], [eps],
                        [x, x_add, w.weight, w.bias, res, y, ln[0] if ln else None, ln[1] if ln else None, ln_out])

    def layernorm(self, x, g, b, y, *, M, C):
        return self.add(LAYERNORM, 0, [M, C], [], [x, g, b, y])

    def query_init(self, obj_mem, y, *, rows, C):
        return self.add(QUERY_INIT, 0, [rows, C], [], [obj_mem, y])

    def query_init2(self, obj_mem, query, query_emb, *, rows, w_init, res_init, w_emb, res_emb, zero=None):
        """QUERY_INIT and the two linears that consume it in one launch (C = 256, 16 summaries per object).
        zero = tensor: cleared as a side job (the fixed-point accumulators of the transformer blocks behind; size % 16 bytes == 0)."""
        assert w_init.kd == 256 and w_init.n == 256 and w_emb.kd == 256 and w_emb.n == 256 and rows % 16 == 0
        nz = 0
        if zero is not None:
            nb = zero.numel() * zero.element_size()
            assert nb % 16 == 0 and zero.is_contiguous()
            nz = nb // 16
        return self.add(QUERY_INIT, 1, [rows, 256, nz], [], [obj_mem, query, query_emb, w_init.weight, w_init.bias, res_init,
                                                             w_emb.weight, w_emb.bias, res_emb, zero])

    def aux_mask(self, logits, fg, nfg, *, K, HW):
        self.memset32(nfg, K, 0)
        return self.add(AUX_MASK, 0, [K, HW], [], [logits, fg, nfg])

    @staticmethod
    def _proj(proj):
        """Fused-projection operands of the attention ops: proj = dict(x, W (PackedLinear), emb=None, ln=(gamma, beta) | None,
        ln_out=None, ldx=256) -> (ldx, [ln_out], [W.weight, W.bias, emb, gamma, beta])."""
        ln = proj.get('ln') or (None, None)
        assert proj['W'].kd == 256
        return proj.get('ldx', 256), proj.get('ln_out'), [proj['W'].weight, proj['W'].bias, proj.get('emb'), ln[0], ln[1]]

    QACC_SCALE = 4294967296.0    # fixed-point scale of the accumulators of the query chain (csrc/qchain.hip)

    @staticmethod
    def _proj_extras(flags, ints, ptrs, acc_in, out_proj):
        """acc_in = (acc int64 [K*Q, 256], bias | None): the rows are x + bias + acc / 2^32 (flags&4: p10, p11) -- acc holds the products
        of the launch in front, summed over its blocks in fixed point.
        out_proj = (PackedLinear Wo [256,256], acc int64 [K*Q, 256]): the output projection runs inside the launch, per head, and is
        ADDED to acc (flags&8: p12, p13; cleared beforehand, e.g. by QUERY_INIT); its bias is left to the consumer (acc_in=(acc, Wo.bias))."""
        ints = list(ints) + [0] * (9 - len(ints))
        ptrs = list(ptrs) + [None] * (14 - len(ptrs))
        if acc_in is not None:
            assert acc_in[0].dtype == torch.int64
            flags |= 4
            ptrs[10], ptrs[11] = acc_in[0], acc_in[1]
        if out_proj is not None:
            assert out_proj[0].kd == 256 and out_proj[0].n == 256 and out_proj[1].dtype == torch.int64
            flags |= 8
            ptrs[12], ptrs[13] = out_proj[0].weight, out_proj[1]
        return flags, ints, ptrs

    def attn_q2p(self, q, kv, fg, nfg, y, *, K, Q, HW, C, heads, ldkv, voff, logits=None, proj=None, acc_in=None, out_proj=None, q_pre=None, hstride=None,
                 clip_objects=None):
        """logits given: the foreground mask is derived inside the kernel from the mask_pred logits (AUX_MASK fused; fg / nfg unused).
        proj given (needs logits): q = (LN(x) + emb) Wq^T + b is computed inside the launch from the unprojected rows proj['x'].
        out_proj (needs proj; chain form, see _proj_extras): y is not written; acc_in optional.
        q_pre (chain form, instead of proj): q f32 [K*Q, 256], already projected and scaled by 1/sqrt(32) -- by the ATTN_P2Q launch of the
        previous transformer block (attn_p2q(next_q=...)).
        clip_objects (chain form, ABI 4): objects per clip when the K objects are those of several clips in lock step (i9); a sequence: the
        clips' own counts (the mixed form, i10)."""
        hs = 0 if hstride in (None, C // heads) else hstride   # chain form only: elements between the heads' k (and v) inside a pixel row (i8)
        mixed = []
        if clip_objects is not None and not isinstance(clip_objects, int):
            assert out_proj is not None and sum(clip_objects) == K and len(clip_objects) > 1, 'clips in lock step need the chain form'
            mixed, clip_objects = [pack_counts(clip_objects)], None
        kg = 0 if clip_objects in (None, K) else int(clip_objects)
        assert kg == 0 or (out_proj is not None and K % kg == 0), 'clips in lock step need the chain form'
        if q_pre is not None:
            assert proj is None and acc_in is None and out_proj is not None and logits is not None
            flags, ints, ptrs = self._proj_extras(3 | 16, [K, Q, HW, C, heads, ldkv, voff, 256], [q_pre, kv, logits, None, None], None, out_proj)
            ints[8] = hs
            return self.add(ATTN_Q2P, flags, ints + [kg] + mixed, [], ptrs)
        if proj is not None:
            assert logits is not None
            ldx, ln_out, tail = self._proj(proj)
            assert out_proj is not None or acc_in is None, 'the chain form of ATTN_Q2P needs out_proj'
            flags, ints, ptrs = self._proj_extras(3, [K, Q, HW, C, heads, ldkv, voff, ldx], [proj['x'], kv, logits, ln_out, y] + tail, acc_in, out_proj)
            assert hs == 0 or out_proj is not None, 'a head stride needs the chain form'
            ints[8] = hs
            return self.add(ATTN_Q2P, flags, ints + [kg] + mixed, [], ptrs)
        assert acc_in is None and out_proj is None
        if logits is not None:
            return self.add(ATTN_Q2P, 1, [K, Q, HW, C, heads, ldkv, voff], [], [q, kv, logits, None, y])
        return self.add(ATTN_Q2P, 0, [K, Q, HW, C, heads, ldkv, voff], [], [q, kv, fg, nfg, y])

    def attn_self(self, qk, v, y, *, K, Q, C, heads, ldqk=0, ldv=0, proj=None, acc_in=None, out_proj=None):
        """proj given: q | k | v = packed in-projection of (LN(x) + emb | LN(x) + emb | LN(x)) computed inside the launch.
        out_proj (needs proj; chain form): y is not written; acc_in optional."""
        if proj is not None:
            ldx, ln_out, tail = self._proj(proj)
            assert out_proj is not None or acc_in is None, 'the chain form of ATTN_SELF needs out_proj'
            flags, ints, ptrs = self._proj_extras(2, [K, Q, C, heads, 0, 0, ldx], [proj['x'], None, y, ln_out, None] + tail, acc_in, out_proj)
            return self.add(ATTN_SELF, flags, ints, [], ptrs)
        assert acc_in is None and out_proj is None
        return self.add(ATTN_SELF, 0, [K, Q, C, heads, ldqk, ldv], [], [qk, v, y])

    def attn_p2q(self, q, kq, vq, y, *, K, Q, HW, C, heads, ldq, ldkv=0, proj=None, acc_in=None, next_q=None, out=None):
        """proj given: k | v of the object queries = packed [k | v] projection of (x + emb | x) computed inside the launch.
        acc_in (needs proj): chain form.  next_q = dict(ln=(gamma, beta), W=PackedLinear Wq, q_out, xn_out) (chain form): extra blocks project
        the NEXT transformer block's ATTN_Q2P queries from the same rows: xn_out = LN(x_eff), q_out = ((xn_out + emb) Wq^T + b) / sqrt(32).
        out = dict(Wo=weights.out_proj_blob(...), res=bf16 [K, HW, 256]) (chain form): y = res + Wo . attention + bias -- the 1x1 conv behind
        the attention (read_from_query's out_proj, object_transformer.py:66-70) inside the launch; the attention itself is not stored."""
        if proj is not None:
            ldx, _, tail = self._proj(proj)
            flags, ints, ptrs = self._proj_extras(2, [K, Q, HW, C, heads, ldq, ldkv, ldx], [q, proj['x'], None, y, None] + tail[:3], acc_in, None)
            if out is not None:
                assert acc_in is not None and out['Wo'].dtype == torch.uint8 and out['Wo'].numel() == 256 * 256 * 2 + 256 * 4
                flags |= 32
                ptrs[2], ptrs[4] = out['Wo'], out['res']
            if next_q is not None:
                assert acc_in is not None and next_q['W'].kd == 256 and next_q['W'].n == 256
                flags |= 16
                ptrs = ptrs + [None] * (16 - len(ptrs))
                ptrs[8], ptrs[9] = next_q['ln']
                ptrs[12], ptrs[13], ptrs[14], ptrs[15] = next_q['W'].weight, next_q['W'].bias, next_q['q_out'], next_q['xn_out']
            return self.add(ATTN_P2Q, flags, ints, [], ptrs)
        assert acc_in is None
        return self.add(ATTN_P2Q, 0, [K, Q, HW, C, heads, ldq, ldkv], [], [q, kq, vq, y])

    def qffn(self, x, x_out, acc_out, *, rows, ln, W1, W2, acc_in=None, hid_slice=64):
        """FFN of a transformer block in one launch: acc_out += relu(LN(x_eff) W1^T + b1) W2^T in fixed point, summed over the FF / hid_slice
        blocks of an object; x_eff = x (+ acc_in) is written to x_out.  W2's bias is left to the consumer (acc_in=(acc_out, W2.bias))."""
        FF = W1.n
        assert W1.kd == 256 and W2.kd == FF and W2.n == 256 and FF % hid_slice == 0 and hid_slice in (64, 128) and rows % 16 == 0
        assert acc_out.dtype == torch.int64
        ints = [rows, FF, hid_slice]
        ptrs = [x, x_out, ln[0], ln[1], W1.weight, W1.bias, W2.weight, acc_out] + [None] * 6
        if acc_in is not None:
            assert acc_in[0].dtype == torch.int64
            ptrs[10], ptrs[11] = acc_in[0], acc_in[1]
        return self.add(QFFN, 0, ints, [], ptrs)

    def summarize(self, feat, wl, m16, y, *, K, HW, C, Q, scratch=None, feat_f32=False, ldf=None, ldw=None):
        """feat_f32 / ldf / ldw: the features in fp32 with a row stride of ldf elements, the weight logits with a row stride of ldw (both
        live in one conv output [feature | logits]); default: bf16 [K*HW, C] and f32 [K*HW, Q]."""
        if scratch is None:
            scratch = torch.zeros((K, -(-HW // 128), Q, C + 1), dtype=torch.float32, device=m16.device)
        return self.add(SUMMARIZE, 1 if feat_f32 else 0, [K, HW, C, Q, C if ldf is None else ldf, Q if ldw is None else ldw], [], [feat, wl, m16, y, scratch])

    def add_pe(self, x, pe, y, *, B, n):
        return self.add(ADD_PE, 0, [B, n], [], [x, pe, y])

    def key_prep(self, key, aux, hi, lo, sc, *, n, query):
        return self.add(KEY_PREP, (1 | KEYPREP_LOOP) if query else 0, [n], [], [key, aux, hi, lo, sc])

    AFF_CSTRIDE = 32          # ints between the candidate counters of consecutive queries (one cache line each)

    def aff_score(self, Ahi, Alo, scale, Bhi, Blo, c, out, cand_val, cand_idx, count, *, HW, HWp, ranges, cap, mode, gmax_precedes_tau=False, nq=None, dma=None,
                  frames=1, extra_lds_kb=0, prio=False, banks=None):
        """gmax_precedes_tau (mode 1): `out` (= tau) sits right behind the [HWp, Gld] maxima of pass 0 in memory; the kernel then
        skips every (tile, 16-query set) that cannot hold a candidate.  nq: 16-query column sets per wave (1, 2 -- the default: aff_score_kernel;
        4: aff_score4_kernel; every choice computes the same bits); dma: the LDS-DMA kernel (aff_score4_kernel) also for 2 sets per wave.  frames > 1: the query operands of that many frames, HWp rows each (HW real ones), stacked -- every
        per-query array (c, maxima, tau, candidate lists, counters) is then indexed by the stacked row.
        banks = (table, n) (clips in lock step, ABI 4): stacked frame e reads bank e % n -- table: u64 [n, 3] = the (A_hi, A_lo, scale) bases of the
        banks, which share the token ranges (Ahi / Alo / scale are then ignored); needs nq = 2 and HWp % 128 == 0."""
        ranges = [(s, n) for (s, n) in ranges if n > 0]
        assert 1 <= len(ranges) <= 3
        G = sum(-(-n // 16) for _, n in ranges)
        ints = [HW, HWp, len(ranges)]
        for r in range(3):
            ints += list(ranges[r]) if r < len(ranges) else [0, 0]
        ints += [G, cap, mode, 2 if nq is None else nq, 0, int(extra_lds_kb), int(bool(dma))]
        if frames > 1:
            ints[1] = frames * HWp
            ints += [HWp]
        ptrs = [Ahi, Alo, scale, Bhi, Blo, c, out, cand_val, cand_idx, count]
        flags = (1 if (gmax_precedes_tau and mode == 1) else 0) | (F_AFF_PRIO if prio else 0)
        if banks is not None:
            assert frames > 1 and frames % banks[1] == 0 and ints[12] == 2 and HWp % 128 == 0
            ints += [banks[1]]
            ptrs += [None, banks[0]]
            flags |= 4
        return self.add(AFF_SCORE, flags, ints, [], ptrs)

    def aff_select(self, gmax, tau, *, HW, HWp, G, top_k, clear_count=None, ticks=(), zero=None, frames=1, prio=False):
        """clear_count: pass 1's candidate counters, zeroed here; ticks: up to two (life, n) ranges advanced by one (USAGE_TICK);
        zero = (buffer, n): f32 range cleared instead (excludes ticks: the usage side buffer of a look-ahead read-out).
        frames > 1: stacked queries, see aff_score."""
        if zero is not None:
            assert not ticks
            return self.add(AFF_SELECT, 1 | SELECT_COARSE | (F_AFF_PRIO if prio else 0), [HW, HWp, G, top_k, zero[1], 0, frames], [], [gmax, tau, clear_count, zero[0], None])
        ticks = list(ticks) + [(None, 0)] * (2 - len(ticks))
        assert len(ticks) == 2
        return self.add(AFF_SELECT, SELECT_COARSE | (F_AFF_PRIO if prio else 0), [HW, HWp, G, top_k, ticks[0][1], ticks[1][1], frames], [], [gmax, tau, clear_count, ticks[0][0], ticks[1][0]])

    def aff_readout(self, cand_val, cand_idx, count, vptrs, usage, y, overflow, *, HW, cap, top_k, K, CV, frames=1, HWp=0, usage_stride=0, prio=False, banks=1, usage_fx=False):
        """frames > 1: stacked queries (HWp rows per frame, see aff_score); frame f's read-out goes to y[f] ([frames, K, HW, CV]) and its
        usage to usage + f * usage_stride counters.  banks > 1: frame f gathers from bank f % banks -- vptrs: u64 [banks, K].
        usage_fx: the usage counters are unsigned 64-bit fixed point (2^-40) instead of f32 -- integer atomics, sums independent of the order of arrival."""
        assert banks == 1 or frames % banks == 0
        return self.add(AFF_READOUT, (F_AFF_PRIO if prio else 0) | (1 if usage_fx else 0), [HW, cap, top_k, K, CV, frames, HWp, usage_stride, banks], [], [cand_val, cand_idx, count, vptrs, usage, y, overflow])

    def memset32(self, dst, n, value=0):
        return self.add(MEMSET32, 0, [n, value], [], [dst])

    def bank_write(self, copies=(), fills=()):
        """One launch for the contiguous copies [(src, dst, nbytes)] (<= 6) and 32-bit fills [(dst, words, pattern)] (<= 2) of a memory
        insertion; more of either spill into further launches."""
        copies, fills = list(copies), list(fills)
        idx = None
        while copies or fills:
            c, copies = copies[:6], copies[6:]
            fl, fills = fills[:2], fills[2:]
            ints, ptrs = [0] * 10, [0] * 14
            for s, (src, dst, nbytes) in enumerate(c):
                assert nbytes % 4 == 0 and nbytes > 0
                ints[s], ptrs[2 * s], ptrs[2 * s + 1] = nbytes // 4, src, dst
            for t, (dst, words, pattern) in enumerate(fl):
                ints[6 + t], ints[8 + t], ptrs[12 + t] = words, pattern, dst
            idx = self.add(BANK_WRITE, 0, ints, [], ptrs)
        return idx

    def copy2d(self, src, dst, *, rows, rowbytes, src_stride, dst_stride, clips=None):
        """clips (the mixed form, i4): the object counts of the clips of a lock-step group -- destination row r (an object) copies the source
        row of its CLIP: a per-clip map expanded to one map per object (16-byte granularity)."""
        assert rowbytes % 4 == 0 and src_stride % 4 == 0 and dst_stride % 4 == 0
        if clips is not None:
            assert sum(clips) == rows and rowbytes % 16 == 0 and src_stride % 16 == 0 and dst_stride % 16 == 0
            return self.add(COPY2D, 0, [rows, rowbytes, src_stride, dst_stride, pack_counts(clips)], [], [src, dst])
        return self.add(COPY2D, 0, [rows, rowbytes, src_stride, dst_stride], [], [src, dst])

    def axpy(self, x, y, *, n, a=1.0):
        return self.add(AXPY, 0, [n], [a], [x, y])

    def usage_tick(self, life, n, life2=None, n2=0, use=None, delta=None, n_use=0, delta_fx=False, clear_delta=False):
        """life[:n] += 1, life2[:n2] += 1, use[:n_use] += delta[:n_use] -- one launch (any part may be absent).  delta_fx: delta holds the unsigned
        64-bit fixed-point sums (2^-40) of AFF_READOUT(usage_fx=True); clear_delta (with delta_fx): and is zero again afterwards."""
        assert delta_fx or not clear_delta
        return self.add(USAGE_TICK, (1 if delta_fx else 0) | (2 if clear_delta else 0), [n, n2, n_use], [], [life, life2, use, delta])

    RS_SPLIT = 16             # chunks of the all-pairs rank count (csrc/bank.hip)

    def rank_select(self, use, life, order, *, n, k, scratch=None, gathers=(), zero=None):
        """scratch: i32 [16 * n] partial ranks (allocated here when not given); gathers: up to two (src, dst, row bytes) -- dst[r] =
        src[order[r]] for r < k, done by the launch that scatters the order; zero = (u32 buffer, words) cleared by that launch."""
        if scratch is None:
            scratch = torch.empty((self.RS_SPLIT * n,), dtype=torch.int32, device=use.device)
            self.keep.append(scratch)
        gathers = list(gathers) + [(None, None, 0)] * (2 - len(gathers))
        assert len(gathers) == 2 and all(g[2] % 16 == 0 for g in gathers)
        z = zero if zero is not None else (None, 0)
        return self.add(RANK_SELECT, 0, [n, k, gathers[0][2] // 4, gathers[1][2] // 4, z[1]], [],
                        [use, life, order, scratch, gathers[0][0], gathers[0][1], gathers[1][0], gathers[1][1], z[0]])

    def gather_rows(self, src, order, dst, *, k, rowbytes, src_stride, dst_stride):
        return self.add(GATHER_ROWS, 0, [k, rowbytes, src_stride, dst_stride], [], [src, order, dst])

    @staticmethod
    def consol_lds(n):
        """Row length of the similarity matrix of a consolidation: n rounded up to a multiple of 32."""
        return -(-n // 32) * 32

    def consol_aff(self, ckey, cshr, pkey, psel, S, colmax, *, n, P):
        """S f32 [P, consol_lds(n)] (similarities, -inf in the padding), colmax u32 [P] (cleared by the caller)."""
        return self.add(CONSOL_AFF, 0, [n, P, self.consol_lds(n)], [], [ckey, cshr, pkey, psel, S, colmax])

    @staticmethod
    def consol_scratch_floats(n, P, C, K):
        nchunk = -(-OpList.consol_lds(n) // 256)
        return nchunk * (K * P * C + 2 * P)

    def consol_read(self, S, colmax, vptrs, cshr, scratch, out_shr, *, n, P, C, K, src, dst):
        return self.add(CONSOL_READ, 0, [n, P, C, K, self.consol_lds(n), src, dst], [], [S, colmax, vptrs, cshr, scratch, out_shr])

    def prob_to_id(self, prob, lut, out, *, P, H, W, plane, ldrow, out_hw=None, png=None):
        """out dtype picks the kernel: uint8 / int32 / int64.  ABI 7 (include/cutie_hip.h): out_hw = (OH, OW) -- the ids of the planes
        resampled bilinearly to that size (out [OH, OW], uint8 / int32) without the resampled probabilities in memory, bit-identical to
        resize() + prob_to_id(); png = (stream, status, scratch) -- the uint8 ids also leave as the zlib stream of a PNG (png_deflate)."""
        code = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}[out.dtype]
        ints = [P, H, W, plane, ldrow]
        if out_hw is not None:
            code |= 4
            ints += [int(out_hw[0]), int(out_hw[1])]
        if png is None:
            return self.add(PROB_TO_ID, code, ints, [], [prob, lut, out])
        stream, status, scratch = png
        ints += [0] * (7 - len(ints)) + [stream.numel(), scratch.numel()]
        return self.add(PROB_TO_ID, code | 8, ints, [], [prob, lut, out, stream, status, scratch])

    MERGE_MAX_SOURCES = 8     # CUTIE_MERGE_MAX_SOURCES (include/cutie_hip.h)
    MERGE_TABLES = 64         # cached table pairs (a frame-slot pool hands a member's planes out at a few addresses in turn)
    _merge_tables = {}        # (device, stream, ((data_ptr, shape, strides), ...)) -> (u64 [S] plane pointers, i32 [S, 4] geometry)

    @classmethod
    def merge_tables(cls, probs):
        """The two device tables of a merge (PROB_TO_ID flags&16): plane pointers and (H, W, plane stride, row stride) per source.  They
        change when a buffer changes, not per frame: cached per (data_ptr, shape, strides) of every source -- and per stream: a table
        that is dropped goes back to the allocator of the stream that built it, behind the launches that read it."""
        dev = probs[0].device
        sig = tuple((t.data_ptr(), tuple(t.shape), tuple(t.stride())) for t in probs)
        key = (str(dev), torch.cuda.current_stream(dev).cuda_stream if dev.type == 'cuda' else 0, sig)
        tabs = cls._merge_tables.get(key)
        if tabs is None:
            while len(cls._merge_tables) >= cls.MERGE_TABLES:
                cls._merge_tables.pop(next(iter(cls._merge_tables)), None)
            ptrs = torch.from_numpy(np.array([t.data_ptr() for t in probs], dtype=np.uint64).view(np.int64)).to(dev)
            geom = torch.tensor([[t.shape[1], t.shape[2], t.stride(0), t.stride(1)] for t in probs], dtype=torch.int32).to(dev)
            tabs = cls._merge_tables[key] = (ptrs, geom)
        return tabs

    def prob_to_id_merged(self, probs, lut, out, *, out_hw, png=None):
        """PROB_TO_ID flags 4 | 16 (ABI 8, include/cutie_hip.h): the ids of S sources merged -- probs = list of f32 [P, h_s, w_s] (any
        plane / row strides, last dimension contiguous: the un-padded views `step` returns are read in place), every one resampled
        bilinearly to out_hw, quantised like (x * 255).to(uint8) and summed as integers; out [OH, OW] uint8 / int32 = lut[first largest
        sum].  png = (stream, status, scratch) as in prob_to_id.  The caller keeps the sources alive until the launch has run."""
        S = len(probs)
        if not 1 <= S <= self.MERGE_MAX_SOURCES:
            raise ValueError(f'prob_to_id_merged: {S} sources, 1 <= S <= {self.MERGE_MAX_SOURCES}')
        P = int(probs[0].shape[0])
        for t in probs:
            if t.dim() != 3 or t.dtype != torch.float32 or t.shape[0] != P or t.stride(2) != 1 or t.device != probs[0].device or t.shape[1] < 1 or t.shape[2] < 1:
                raise ValueError('prob_to_id_merged: sources are f32 [P, h, w] of one P and device with a contiguous last dimension')
            if max(t.stride(0), t.stride(1)) >= 1 << 31:
                raise ValueError('prob_to_id_merged: strides are 32-bit')
        if out.dtype not in (torch.uint8, torch.int32):
            raise ValueError('prob_to_id_merged: out is uint8 or int32')
        OH, OW = int(out_hw[0]), int(out_hw[1])
        if tuple(out.shape) != (OH, OW) or not out.is_contiguous():
            raise ValueError('prob_to_id_merged: out is a contiguous [OH, OW]')
        code = {torch.uint8: 0, torch.int32: 1}[out.dtype] | 4 | 16
        ptrs, geom = self.merge_tables(probs)
        self.keep.extend(probs)
        ints = [P, 0, 0, 0, 0, OH, OW, 0, 0, S]
        if png is None:
            return self.add(PROB_TO_ID, code, ints, [], [ptrs, lut, out, None, None, None, geom])
        stream, status, scratch = png
        ints[7], ints[8] = stream.numel(), scratch.numel()
        return self.add(PROB_TO_ID, code | 8, ints, [], [ptrs, lut, out, stream, status, scratch, geom])

    @staticmethod
    def png_capacity(H, W):
        """Bytes that hold the zlib stream of ANY uint8 plane [H, W]: with the fixed Huffman codes a filtered byte costs at most 9 bits;
        2 bytes header, block header + end of block (10 bits), 4 bytes Adler-32; rounded up to a multiple of 4."""
        return -(-(-(-((W + 1) * H * 9 + 10) // 8) + 6) // 4) * 4

    @staticmethod
    def png_scratch_words(H, W):
        """int32 words of the scratch of png_deflate: per row 4 words of bookkeeping and the row's bits (csrc/png.hip png_row_words)."""
        return H * (4 + (9 * (W + 1) + 31) // 32 + 2)

    def png_deflate(self, ids, stream, status, scratch, *, H, W):
        """PROB_TO_ID flags&8 on its own: ids uint8 [H, W] (contiguous) -> stream uint8 [capacity] = the complete zlib stream of the
        PNG-filtered plane (filter 0), status int32 [4] = (stream bytes, Adler-32, error bits: 1 = the capacity is too small and nothing
        was written, 0).  scratch int32 [>= png_scratch_words(H, W)], 16-byte aligned.  cutie_amd/inference/utils/png.py wraps the stream."""
        return self.add(PROB_TO_ID, 8, [0, H, W, 0, 0, 0, 0, stream.numel(), scratch.numel()], [], [None, None, ids, stream, status, scratch])

    PNG_PHOTO_ROW_LIMIT = 16384   # L = W * B + 1 (csrc/png_photo.hip PPH_ROW_LIMIT): every match distance inside DEFLATE's window
    PNG_PHOTO_BAND = 32           # rows per DEFLATE block (PPH_R)

    @classmethod
    def png_photo_fits(cls, W, B):
        """Does a row of W pixels of B bytes fit the row limit of png_photo?"""
        return W * B + 1 <= cls.PNG_PHOTO_ROW_LIMIT

    @classmethod
    def png_photo_capacity(cls, H, W, B):
        """Bytes that hold the zlib stream of ANY image of H x W pixels of B bytes: a block is never longer than its fixed-code form, in
        which a filtered byte costs at most 9 bits; 10 bits of header and end-of-block per block of 32 rows; 2 bytes header, 4 bytes
        Adler-32; rounded up to a multiple of 4."""
        nb = -(-H // cls.PNG_PHOTO_BAND)
        return -(-(-(-(9 * H * (W * B + 1) + 10 * nb) // 8) + 6) // 4) * 4

    @classmethod
    def png_photo_scratch_words(cls, H, W, B):
        """int32 words of the scratch of png_photo (csrc/png_photo.hip pph_layout): 4 per row, 1024 per block of 32 rows (counts, codes,
        header), the filtered bytes [H, L] and a 16-bit record per filtered byte, each rounded up to 4 words."""
        L, nb = W * B + 1, -(-H // cls.PNG_PHOTO_BAND)
        up4 = lambda v: (v + 3) & ~3
        return 4 * H + 1024 * nb + up4(-(-H * L // 4)) + up4(-(-H * L // 2))

    def png_photo(self, src, stream, status, scratch, *, last=None, ldrow=None):
        """PROB_TO_ID flags == 16384 (ABI 11, form added; include/cutie_hip.h): the complete zlib stream of a PNG with scanline filters
        and dynamic Huffman codes.  ``src`` uint8 [H, W] (a plane) or [H, W, 3] (packed pixels, row stride ``ldrow`` bytes, default the
        tensor's), ``last`` an optional uint8 [H, W] plane that becomes the last channel: B = 1 (L), 2 (LA), 3 (RGB) or 4 (RGBA) bytes per
        pixel, interleaved inside the launch.  ``stream`` uint8 [capacity] (4-byte aligned; png_photo_capacity holds any image);
        ``status`` int32 [4] = (stream bytes, Adler-32, error bits: 1 = the capacity is too small and nothing was written, 0);
        ``scratch`` int32 [>= png_photo_scratch_words(H, W, B)], 16-byte aligned.  W * B + 1 <= PNG_PHOTO_ROW_LIMIT.
        cutie_amd/inference/utils/png.py wraps the stream (assemble_image)."""
        _need_form(_lib.has_png_photo, 'no filtered PNG stream, PROB_TO_ID flags == 16384')
        if src.dtype != torch.uint8 or src.dim() not in (2, 3) or (src.dim() == 3 and (src.shape[2] != 3 or src.stride(1) != 3)) or src.stride(-1) != 1:
            raise ValueError(f'png_photo: src is uint8 [H, W] or [H, W, 3] with packed pixels, not {src.dtype} {tuple(src.shape)} strides {src.stride()}')
        H, W, c0 = int(src.shape[0]), int(src.shape[1]), 3 if src.dim() == 3 else 1
        if H < 1 or W < 1:
            raise ValueError(f'png_photo: an image of {H} x {W}')
        ld0 = int(src.stride(0) if ldrow is None else ldrow)
        if ld0 < W * c0:
            raise ValueError(f'png_photo: a row stride of {ld0} bytes below the row\'s {W * c0}')
        B = c0 + (1 if last is not None else 0)
        if last is not None and (last.dtype != torch.uint8 or tuple(last.shape) != (H, W) or last.stride(1) != 1 or last.stride(0) < W):
            raise ValueError(f'png_photo: last is a uint8 [{H}, {W}] plane with contiguous rows')
        if not self.png_photo_fits(W, B):
            raise ValueError(f'png_photo: a row of {W} pixels of {B} bytes: W * B + 1 <= {self.PNG_PHOTO_ROW_LIMIT}')
        if 9 * H * (W * B + 1) + 10 * -(-H // self.PNG_PHOTO_BAND) + 64 >= 1 << 31:
            raise ValueError(f'png_photo: {H} x {W} x {B} exceeds 2^31 stream bits')
        if stream.dtype != torch.uint8 or not stream.is_contiguous() or stream.data_ptr() % 4:
            raise ValueError('png_photo: stream is a contiguous uint8 buffer, 4-byte aligned')
        if status.dtype != torch.int32 or status.numel() != 4 or not status.is_contiguous():
            raise ValueError('png_photo: status is a contiguous int32 [4]')
        need = self.png_photo_scratch_words(H, W, B)
        if scratch.dtype != torch.int32 or not scratch.is_contiguous() or scratch.numel() < need or scratch.data_ptr() % 16:
            raise ValueError(f'png_photo: scratch is a contiguous int32 of at least {need} words, 16-byte aligned')
        for name, t in (('last', last), ('stream', stream), ('status', status), ('scratch', scratch)):
            if t is not None and t.device != src.device:
                raise ValueError(f'png_photo: {name} is on {t.device}, src on {src.device}')
        return self.add(PROB_TO_ID, 16384, [0, H, W, c0, ld0, int(last.stride(0)) if last is not None else 0, 0, stream.numel(),
                                            min(scratch.numel(), (1 << 31) - 1)], [],
                        [None, None, src, stream, status, scratch, last])

    GUIDED_MAX_RADIUS = 64    # csrc/guided.hip GF_RMAX
    GUIDED_MAX_PLANES = 16    # GF_MAXS: planes per op; the host splits more over several ops
    GUIDED_THREADS = 256      # GF_T: the columns a block holds, both halos of GUIDED_MAX_RADIUS included
    GUIDED_TILE_X = 128       # GF_TX: output columns per block
    GUIDED_TILE_Y = 64        # GF_TY: output rows per block (the column sums are rebuilt at every multiple of it)
    GUIDED_EPS_MIN, GUIDED_EPS_MAX = 1e-6, 1.0

    @staticmethod
    def guided_scratch_words(S, H, W):
        """int32 words of the scratch of guided_filter: the four fixed-point coefficients of every plane and pixel."""
        return 4 * S * H * W

    def guided_filter(self, guide, planes, out, scratch, *, radius, eps, last=None, ldrow=None):
        """PROB_TO_ID flags == 32768 (ABI 11, form added; include/cutie_hip.h): the colour guided filter (He, Sun, Tang) of uint8 planes
        under a uint8 guide -- every plane is fitted, per window of (2 radius + 1)^2 pixels clipped at the frame, as an affine function of
        the guide's RGB, and the fits are averaged: the planes' edges move onto the guide's.  ``guide`` uint8 [H, W, 3] (packed pixels,
        row stride ``ldrow`` bytes, default the tensor's, any alignment); ``planes`` uint8 [S0, H, W] (contiguous pixels, any row and
        plane strides, any alignment) or None; ``last`` an optional uint8 [H, W] plane filtered as plane S0 (a matte that lives in a
        tensor of its own); S = S0 + (last is not None), 1 <= S <= GUIDED_MAX_PLANES.  ``out`` uint8 [S, H, W] contiguous, overlapping no
        input.  ``radius`` 1 .. GUIDED_MAX_RADIUS; ``eps`` GUIDED_EPS_MIN .. GUIDED_EPS_MAX in units of the guide scaled to [0, 1]
        (carried as a float32).  ``scratch`` int32 [>= guided_scratch_words(S, H, W)].  Integer sums and a float64 solve in a fixed order:
        the bytes are those of tests/guided_ref.py model, whatever the launch shape."""
        _need_form(_lib.has_guided_filter, 'no guided filter, PROB_TO_ID flags == 32768')
        who = 'guided_filter'
        if guide.dtype != torch.uint8 or guide.dim() != 3 or guide.shape[2] != 3 or guide.stride(2) != 1 or guide.stride(1) != 3:
            raise ValueError(f'{who}: guide is uint8 [H, W, 3] with packed pixels, not {guide.dtype} {tuple(guide.shape)} strides {guide.stride()}')
        H, W = int(guide.shape[0]), int(guide.shape[1])
        if H < 1 or W < 1 or H * W >= 1 << 31:
            raise ValueError(f'{who}: a frame of {H} x {W}: H, W >= 1 and H * W < 2^31')
        ldg = int(guide.stride(0) if ldrow is None else ldrow)
        if ldg < 3 * W:
            raise ValueError(f"{who}: a guide row stride of {ldg} bytes below the row's {3 * W}")
        S0 = 0
        if planes is not None:
            if planes.dtype != torch.uint8 or planes.dim() != 3 or tuple(planes.shape[1:]) != (H, W) or planes.stride(2) != 1:
                raise ValueError(f'{who}: planes is uint8 [S, {H}, {W}] with contiguous pixels, not {planes.dtype} {tuple(planes.shape)} strides {planes.stride()}')
            S0 = int(planes.shape[0])
        if last is not None and (last.dtype != torch.uint8 or tuple(last.shape) != (H, W) or last.stride(1) != 1):
            raise ValueError(f'{who}: last is a uint8 [{H}, {W}] plane with contiguous pixels')
        S = S0 + (1 if last is not None else 0)
        if not 1 <= S <= self.GUIDED_MAX_PLANES:
            raise ValueError(f'{who}: {S} planes, 1 .. {self.GUIDED_MAX_PLANES} (split more over several ops)')
        ldp, ps, ldl = 0, 0, int(last.stride(0)) if last is not None else 0
        if S0:
            ldp, ps = int(planes.stride(1)), int(planes.stride(0))
            if ldp < W or (S0 > 1 and ps < (H - 1) * ldp + W) or ps >= 1 << 31:
                raise ValueError(f'{who}: plane strides {planes.stride()}: rows of at least {W} bytes, planes that do not overlap, below 2^31')
        if last is not None and ldl < W:
            raise ValueError(f"{who}: a row stride of last of {ldl} bytes below the row's {W}")
        radius = int(radius)
        if not 1 <= radius <= self.GUIDED_MAX_RADIUS:
            raise ValueError(f'{who}: radius {radius}, 1 .. {self.GUIDED_MAX_RADIUS}')
        eps = float(eps)
        if not np.float32(self.GUIDED_EPS_MIN) <= np.float32(eps) <= np.float32(self.GUIDED_EPS_MAX):     # as the launcher judges it (NaN fails both)
            raise ValueError(f'{who}: eps {eps}, {self.GUIDED_EPS_MIN} .. {self.GUIDED_EPS_MAX}')
        if out.dtype != torch.uint8 or tuple(out.shape) != (S, H, W) or not out.is_contiguous():
            raise ValueError(f'{who}: out is a contiguous uint8 [{S}, {H}, {W}], not {out.dtype} {tuple(out.shape)}')
        need = self.guided_scratch_words(S, H, W)
        if scratch.dtype != torch.int32 or not scratch.is_contiguous() or scratch.numel() < need:
            raise ValueError(f'{who}: scratch is a contiguous int32 of at least {need} words')
        for name, t in (('planes', planes), ('last', last), ('out', out), ('scratch', scratch)):
            if t is not None and t.device != guide.device:
                raise ValueError(f'{who}: {name} is on {t.device}, guide on {guide.device}')
        spans = [('guide', guide.data_ptr(), (H - 1) * ldg + 3 * W)]
        if S0:
            spans.append(('planes', planes.data_ptr(), (S0 - 1) * ps + (H - 1) * ldp + W))
        if last is not None:
            spans.append(('last', last.data_ptr(), (H - 1) * ldl + W))
        for name, at, n in spans:
            if at < out.data_ptr() + S * H * W and out.data_ptr() < at + n:
                raise ValueError(f'{who}: out overlaps {name}: the filter does not work in place')
        words = int(scratch.numel())
        return self.add(PROB_TO_ID, 32768, [0, H, W, radius, ldg, ldp, ps, words >> 31, words & 0x7fffffff, S0, ldl], [eps],
                        [None, None, guide, out, None, scratch, planes, last])

    REDACT_MODES = {'blur': 0, 'pixelate': 1, 'fill': 2}     # i6 of PROB_TO_ID flags == 65536 (csrc/redact.hip)
    REDACT_MAX_RADIUS = 64    # RD_RMAX, CUTIE_REDACT_MAX_RADIUS
    REDACT_MAX_CELL = 256     # RD_CMAX, CUTIE_REDACT_MAX_CELL
    REDACT_THREADS = 256      # RD_T: the pixel columns a block of a blur pass holds, both halos of the radius included (256 - 2 r of output)
    REDACT_TILE_Y = (32, 64)  # RD_TY_SMALL, RD_TY_LARGE: output rows per block for r <= REDACT_SMALL_RADIUS and above it
    REDACT_SMALL_RADIUS = 16  # RD_R_SMALL

    @classmethod
    def redact_scratch_words(cls, mode, H, W, strength=None):
        """int32 words of the scratch of redact.  ``mode`` 'blur' | 'pixelate' | 'fill' (or its code): blur takes two uint8 RGB images,
        each rounded up to a word; pixelate the column sums [ceil(H / c)][3 W] and the cells' bytes -- for the cell size ``strength``,
        without it for c = 2, which holds every cell size; fill one word that is never touched (a tensor with a pointer)."""
        code = cls.REDACT_MODES.get(mode, mode)
        if code == 0:
            return 2 * -(-3 * H * W // 4)
        if code == 1:
            c = 2 if strength is None else int(strength)
            CY, CX = -(-H // c), -(-W // c)
            return CY * 3 * W + -(-CY * CX * 3 // 4)
        if code == 2:
            return 1
        raise ValueError(f'redact_scratch_words: mode is one of {tuple(cls.REDACT_MODES)}, not {mode!r}')

    def redact(self, frame, weight, out, scratch, *, mode, strength=0, color=(0, 0, 0), invert=False, ldrow=None, ldw=None):
        """PROB_TO_ID flags == 65536 (ABI 11, form added; include/cutie_hip.h): the frame with an effect blended over it under a weight
        plane -- out = (w' e + (255 - w') f + 127) / 255 per byte, w' = ``weight`` (255 - weight with ``invert``), e the effect:
        ``mode`` 'blur' (three box passes of radius ``strength``, 1 .. REDACT_MAX_RADIUS, every pass one 2-D window mean rounded once,
        windows clipped at the frame), 'pixelate' (the rounded mean of the cell of ``strength`` x ``strength`` pixels, 2 ..
        REDACT_MAX_CELL, anchored at the origin) or 'fill' (``color``, three bytes).  ``frame`` uint8 [H, W, 3] (packed pixels, row
        stride ``ldrow`` bytes, default the tensor's, any alignment), ``weight`` uint8 [H, W] (contiguous pixels, row stride ``ldw``,
        default the tensor's), both read only; ``out`` uint8 [H, W, 3] contiguous, overlapping neither; ``scratch`` int32 [>=
        redact_scratch_words(mode, H, W, strength)].  Integers only: the bytes are those of tests/redact_ref.py, whatever the launch shape."""
        _need_form(_lib.has_redact, 'no redacted frames, PROB_TO_ID flags == 65536')
        who = 'redact'
        if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3 or frame.stride(2) != 1 or frame.stride(1) != 3:
            raise ValueError(f'{who}: frame is uint8 [H, W, 3] with packed pixels, not {frame.dtype} {tuple(frame.shape)} strides {frame.stride()}')
        H, W = int(frame.shape[0]), int(frame.shape[1])
        if H < 1 or W < 1 or H * W >= 1 << 31:
            raise ValueError(f'{who}: a frame of {H} x {W}: H, W >= 1 and H * W < 2^31')
        code = self.REDACT_MODES.get(mode)
        if code is None:
            raise ValueError(f'{who}: mode is one of {tuple(self.REDACT_MODES)}, not {mode!r}')
        if isinstance(strength, bool) or int(strength) != strength:
            raise ValueError(f'{who}: strength is an integer, not {strength!r}')
        strength = int(strength)
        if code == 0 and not 1 <= strength <= self.REDACT_MAX_RADIUS:
            raise ValueError(f'{who}: blur radius {strength}, 1 .. {self.REDACT_MAX_RADIUS}')
        if code == 1 and not 2 <= strength <= self.REDACT_MAX_CELL:
            raise ValueError(f'{who}: pixelate cell {strength}, 2 .. {self.REDACT_MAX_CELL}')
        try:
            rgb = [int(v) for v in color]
        except (TypeError, ValueError):
            rgb = []
        if len(rgb) != 3 or any(not 0 <= v <= 255 for v in rgb):
            raise ValueError(f'{who}: color is three bytes (R, G, B), not {color!r}')
        ldf = int(frame.stride(0) if ldrow is None else ldrow)
        if ldf < 3 * W:
            raise ValueError(f"{who}: a frame row stride of {ldf} bytes below the row's {3 * W}")
        if weight.dtype != torch.uint8 or tuple(weight.shape) != (H, W) or weight.stride(1) != 1:
            raise ValueError(f'{who}: weight is a uint8 [{H}, {W}] plane with contiguous pixels, not {weight.dtype} {tuple(weight.shape)} strides {weight.stride()}')
        ldw = int(weight.stride(0) if ldw is None else ldw)
        if ldw < W:
            raise ValueError(f"{who}: a weight row stride of {ldw} bytes below the row's {W}")
        if out.dtype != torch.uint8 or tuple(out.shape) != (H, W, 3) or not out.is_contiguous():
            raise ValueError(f'{who}: out is a contiguous uint8 [{H}, {W}, 3], not {out.dtype} {tuple(out.shape)}')
        need = self.redact_scratch_words(code, H, W, strength)
        if scratch.dtype != torch.int32 or not scratch.is_contiguous() or scratch.numel() < need:
            raise ValueError(f'{who}: scratch is a contiguous int32 of at least {need} words')
        for name, t in (('weight', weight), ('out', out), ('scratch', scratch)):
            if t.device != frame.device:
                raise ValueError(f'{who}: {name} is on {t.device}, frame on {frame.device}')
        spans = [('frame', frame.data_ptr(), (H - 1) * ldf + 3 * W), ('weight', weight.data_ptr(), (H - 1) * ldw + W)]
        for mine, at0, n0 in (('out', out.data_ptr(), 3 * H * W), ('scratch', scratch.data_ptr(), 4 * need)):
            for name, at, n in spans:
                if at < at0 + n0 and at0 < at + n:
                    raise ValueError(f'{who}: {mine} overlaps {name}: the stage does not work in place')
            spans = spans + [(mine, at0, n0)]
        words = int(scratch.numel())
        return self.add(PROB_TO_ID, 65536, [0, H, W, strength, ldf, ldw, code, words >> 31, words & 0x7fffffff, 1 if invert else 0,
                                            rgb[0] | rgb[1] << 8 | rgb[2] << 16], [], [None, None, frame, out, None, scratch, weight])

    RLE_MAX_OBJECTS = 255

    @staticmethod
    def rle_scratch_words(H, W, n_objects):
        """int32 words of the scratch of rle_encode (csrc/rle.hip launch_rle_encode): 1024 words of per-object sums, one word per 1024
        boundaries, the starts per (object, chunk) -- a chunk is <= 256 rows of one column -- and the boundary positions, at most two per
        pixel and one sentinel per object."""
        G = 2 * H * W + n_objects
        return 1024 + -(-(-(-G // 1024)) // 4) * 4 + n_objects * W * -(-H // 256) + G

    def rle_encode(self, ids, objects, stream, table, status, scratch, *, H, W, n_objects):
        """PROB_TO_ID flags == 32 (ABI 9, include/cutie_hip.h): ids uint8 [H, W] (contiguous) -> the COCO compressed-RLE strings (the
        bytes of inference/utils/coco_rle.py encode(ids == objects[k])) of the n_objects <= 255 ids in ``objects`` (int32 on the device,
        distinct, 1 .. 255), back to back in ``stream`` (uint8 [capacity]); table int32 [n_objects, 4] = per object (byte offset, bytes,
        counts, area), 16-byte aligned; status int32 [4] = (bytes of all strings, error bits: 1 = the capacity is too small and nothing
        was written to the stream, counts of all strings, 0); scratch int32 [>= rle_scratch_words(H, W, n_objects)], 16-byte aligned."""
        if not 0 <= n_objects <= self.RLE_MAX_OBJECTS:
            raise ValueError(f'rle_encode: {n_objects} objects, 0 .. {self.RLE_MAX_OBJECTS}')
        return self.add(PROB_TO_ID, 32, [0, H, W, 0, 0, 0, 0, stream.numel(), scratch.numel(), n_objects], [],
                        [None, None, ids, stream, status, scratch, objects, table])

    JF_MAX_RADIUS = 40        # CUTIE_JF_MAX_RADIUS (include/cutie_hip.h): covers 2160 x 3840, where the DAVIS radius is 36
    JF_MAX_OBJECTS = 255

    @staticmethod
    def jf_scratch_words(H, W, n_objects):
        """int32 words of the scratch of jf_counts (csrc/score.hip launch_jf_counts): the boundary bit planes of the prediction and of
        the ground truth per object, one 64-bit word per 64 columns of a row."""
        return 4 * n_objects * H * -(-W // 64)

    def jf_counts(self, pred, gt, objects, counts, scratch=None, *, H, W, radius):
        """PROB_TO_ID flags == 64 (ABI 10, include/cutie_hip.h): pred, gt uint8 [H, W] (contiguous) -> counts int32 [n, 8], WRITTEN by the
        launch: per object of ``objects`` (a sequence of distinct ids 1 .. 254, or an int32 tensor of them on the device, which is not
        inspected) |pred & gt|, |pred | gt|, boundary pixels of pred, of gt, pred boundary pixels within ``radius`` of a gt boundary
        pixel, gt boundary pixels within ``radius`` of a pred one, area of pred, of gt -- the integers of DAVIS J and F
        (inference/utils/davis_metrics.py).  scratch int32 [>= jf_scratch_words(H, W, n)], 16-byte aligned (allocated here when not
        given); counts 16-byte aligned."""
        H, W, radius = int(H), int(W), int(radius)
        n, objs, ids = _object_ids('jf_counts', 'objects', objects)
        if ids is not None:
            if any(v < 1 or v >= 255 for v in ids):
                raise ValueError(f'jf_counts: object ids are 1 .. 254 (0 is the background, 255 the void label), not {ids}')
            if len(set(ids)) != n:
                raise ValueError(f'jf_counts: duplicate object ids in {ids}')
        if not 1 <= n <= self.JF_MAX_OBJECTS:
            raise ValueError(f'jf_counts: {n} objects, 1 .. {self.JF_MAX_OBJECTS}')
        for name, t in (('pred', pred), ('gt', gt)):
            _u8_plane('jf_counts', name, t, (H, W))
        if not 1 <= radius <= self.JF_MAX_RADIUS:
            raise ValueError(f'jf_counts: radius {radius}, 1 .. {self.JF_MAX_RADIUS}')
        if counts.dtype != torch.int32 or counts.numel() != n * 8 or not counts.is_contiguous():
            raise ValueError(f'jf_counts: counts is a contiguous int32 [{n}, 8]')
        need = self.jf_scratch_words(H, W, n)
        if scratch is None:
            scratch = torch.empty(need, dtype=torch.int32, device=pred.device)
            self.keep.append(scratch)
        elif scratch.dtype != torch.int32 or scratch.numel() < need:
            raise ValueError(f'jf_counts: scratch is int32 [>= {need}]')
        if objs is None:
            objs = torch.tensor(ids, dtype=torch.int32).to(pred.device)
            self.keep.append(objs)
        return self.add(PROB_TO_ID, 64, [0, H, W, 0, 0, radius, 0, 0, min(scratch.numel(), (1 << 31) - 1), n], [],
                        [None, None, pred, gt, None, scratch, objs, counts])

    TRACK_MAX_OBJECTS = 255
    TRACK_WORDS = 12          # int32 words of a table row (csrc/tracks.hip TRK_WORDS)

    def track_stats(self, ids_plane, obj_ids, table, prob=None, lut=None):
        """PROB_TO_ID flags == 1024 (ABI 11, form added; include/cutie_hip.h): ids_plane uint8 [H, W] (contiguous) -> table int32 [n, 12],
        WRITTEN by the launch: per object of ``obj_ids`` (a sequence of ints, or an int32 tensor of them on the device, which is not
        inspected) area, xmin, ymin, xmax, ymax, sum of x, sum of y (64-bit pairs, low word first), and from ``prob`` (f32 [P, h, w], any
        plane / row strides, last dimension contiguous: the un-padded view `step` returns is read in place) with ``lut`` (int32 [P] on
        the device, plane -> object id) the number of samples the object's plane won and the sum of q16 of the winning probability
        (64-bit).  Entries outside 1 .. 255 are absent objects, a repeated entry gets the first one's row; an object without a pixel
        has area 0, xmin = W, ymin = H, xmax = ymax = -1.  table 16-byte aligned.  The caller keeps ``prob`` alive until the launch
        has run (the list holds it)."""
        _need_form(_lib.has_track_stats, 'no track statistics, PROB_TO_ID flags == 1024')
        H, W = _u8_plane('track_stats', 'ids_plane', ids_plane)
        n, objs, listed = _object_ids('track_stats', 'obj_ids', obj_ids)
        if not 0 <= n <= self.TRACK_MAX_OBJECTS:
            raise ValueError(f'track_stats: {n} objects, 0 .. {self.TRACK_MAX_OBJECTS}')
        if table.dtype != torch.int32 or table.numel() != n * self.TRACK_WORDS or not table.is_contiguous():
            raise ValueError(f'track_stats: table is a contiguous int32 [{n}, {self.TRACK_WORDS}]')
        if (prob is None) != (lut is None):
            raise ValueError('track_stats: prob and lut come together')
        ints = [0, H, W, 0, 0, 0, 0, 0, 0, n]
        if prob is not None:
            if prob.dim() != 3 or prob.dtype != torch.float32 or prob.stride(2) != 1 or prob.shape[1] < 1 or prob.shape[2] < 1:
                raise ValueError('track_stats: prob is f32 [P, h, w] with a contiguous last dimension')
            P, h, w = (int(v) for v in prob.shape)
            if not 1 <= P <= 256:
                raise ValueError(f'track_stats: {P} probability planes, 1 .. 256')
            if h * w >= 1 << 31 or max(prob.stride(0), prob.stride(1)) >= 1 << 31 or prob.stride(1) < w:
                raise ValueError('track_stats: h * w < 2^31, strides are 32-bit and a row stride covers the row')
            if lut.dtype != torch.int32 or lut.numel() != P or not lut.is_contiguous():
                raise ValueError(f'track_stats: lut is a contiguous int32 [{P}]')
            ints[0], ints[3], ints[4], ints[5], ints[6] = P, int(prob.stride(0)), int(prob.stride(1)), h, w
        if objs is None and n:
            objs = torch.tensor(listed, dtype=torch.int32).to(ids_plane.device)
            self.keep.append(objs)
        return self.add(PROB_TO_ID, 1024, ints, [], [prob, lut, ids_plane, None, None, None, objs if n else None, table if n else None])

    REGION_TILE_H = 16        # the tile of the local labelling (csrc/regions.hip RGN_TH, RGN_TW): components are merged across its seams
    REGION_TILE_W = 64

    @staticmethod
    def region_scratch_words(H, W):
        """int32 words of the region filter's scratch: a label and a size word per pixel."""
        return 2 * H * W

    def region_filter(self, ids_plane, scratch, counts, *, min_region=0, fill_holes=0, connectivity=8):
        """PROB_TO_ID flags == 2048 (ABI 11, form added; include/cutie_hip.h): ids_plane uint8 [H, W] (contiguous, any alignment) is
        rewritten IN PLACE: object components (equal non-zero id, connected under ``connectivity`` 4 | 8) of fewer than ``min_region``
        pixels become 0, then enclosed background components of fewer than ``fill_holes`` pixels get the id left of their first pixel.
        Thresholds 0 and 1 switch a stage off.  ``scratch``: int32, at least ``region_scratch_words(H, W)`` words; ``counts``: int32
        [4], WRITTEN by the launch: islands removed | pixels cleared | holes filled | pixels filled."""
        _need_form(_lib.has_region_filter, 'no region filter, PROB_TO_ID flags == 2048')
        H, W = _u8_plane('region_filter', 'ids_plane', ids_plane)
        min_region, fill_holes, connectivity = int(min_region), int(fill_holes), int(connectivity)
        if min_region < 0 or fill_holes < 0 or max(min_region, fill_holes) >= 1 << 31:
            raise ValueError(f'region_filter: min_region {min_region} and fill_holes {fill_holes} are 32-bit and not negative')
        if connectivity not in (4, 8):
            raise ValueError(f'region_filter: connectivity {connectivity}, 4 or 8')
        if scratch.dtype != torch.int32 or not scratch.is_contiguous() or scratch.numel() < self.region_scratch_words(H, W):
            raise ValueError(f'region_filter: scratch is a contiguous int32 of at least {self.region_scratch_words(H, W)} words')
        if counts.dtype != torch.int32 or counts.numel() != 4 or not counts.is_contiguous():
            raise ValueError('region_filter: counts is a contiguous int32 [4]')
        words = int(scratch.numel())
        return self.add(PROB_TO_ID, 2048, [0, H, W, min_region, fill_holes, connectivity, 0, 0, words & 0x7fffffff, words >> 31], [],
                        [None, None, ids_plane, None, None, scratch, None, counts])

    EDT_MAX_LIMIT = 65536     # CUTIE_EDT_MAX_LIMIT (include/cutie_hip.h): distances are exact below it; radii up to 255
    EDT_MAX_SETS = 16         # CUTIE_EDT_MAX_SETS
    EDT_COL_GROUP = 64        # columns per block of the column pass (csrc/edt.hip EDT_CW)
    EDT_ROW_CHUNK = 32        # least rows per thread of the column pass (EDT_CH; max(EDT_CH, ceil(sqrt(limit))) rows)
    EDT_ROW_SEGMENT = 256     # pixels per block of the row pass (EDT_T)

    @staticmethod
    def edt_scratch_words(S, H, W):
        """int32 words of the scratch of edt_band: one uint16 per set and pixel."""
        return (S * H * W + 1) // 2

    def edt_band(self, ids_plane, sets, scratch, *, band=None, dist2=None, inner=0, outer=0, mid=128, limit=None):
        """PROB_TO_ID flags == 4096 (ABI 11, form added; include/cutie_hip.h): ids_plane uint8 [H, W] (contiguous, any alignment, read
        only) and ``sets`` uint8 [S, 256] on the device (id v is in set s iff sets[s, v] != 0) -> per set the exact squared Euclidean
        distance of every pixel to the nearest pixel of the other class inside the frame, D = min(d2, limit) (``dist2`` int32 [S, H, W])
        and the band byte (``band`` uint8 [S, H, W]): inside the set 255 where D > ``inner`` else ``mid``, outside it ``mid`` where D <=
        ``outer`` else 0.  Either output may be None, not both.  ``limit`` defaults to max(inner, outer) + 1.  ``scratch``: int32, at
        least ``edt_scratch_words(S, H, W)`` words."""
        _need_form(_lib.has_edt_band, 'no distance transform, PROB_TO_ID flags == 4096')
        H, W = _u8_plane('edt_band', 'ids_plane', ids_plane)
        if sets.dtype != torch.uint8 or sets.dim() != 2 or sets.shape[1] != 256 or not sets.is_contiguous():
            raise ValueError(f'edt_band: sets is a contiguous uint8 [S, 256], not {sets.dtype} {tuple(sets.shape)}')
        S = int(sets.shape[0])
        if not 1 <= S <= self.EDT_MAX_SETS:
            raise ValueError(f'edt_band: {S} sets, 1 .. {self.EDT_MAX_SETS} (split more over several ops)')
        inner, outer, mid = int(inner), int(outer), int(mid)
        limit = max(inner, outer) + 1 if limit is None else int(limit)
        if inner < 0 or outer < 0:
            raise ValueError(f'edt_band: inner {inner} and outer {outer} are not negative')
        if not max(inner, outer) < limit <= self.EDT_MAX_LIMIT:
            raise ValueError(f'edt_band: limit {limit}: max(inner, outer) = {max(inner, outer)} < limit <= {self.EDT_MAX_LIMIT}')
        if not 0 <= mid <= 255:
            raise ValueError(f'edt_band: mid {mid} is a byte')
        if band is None and dist2 is None:
            raise ValueError('edt_band: band, dist2 or both')
        for name, t, dtype in (('band', band, torch.uint8), ('dist2', dist2, torch.int32)):
            if t is not None and (t.dtype != dtype or tuple(t.shape) != (S, H, W) or not t.is_contiguous()):
                raise ValueError(f'edt_band: {name} is a contiguous {dtype} [{S}, {H}, {W}], not {t.dtype} {tuple(t.shape)}')
        need = self.edt_scratch_words(S, H, W)
        if scratch.dtype != torch.int32 or not scratch.is_contiguous() or scratch.numel() < need:
            raise ValueError(f'edt_band: scratch is a contiguous int32 of at least {need} words')
        for name, t in (('sets', sets), ('scratch', scratch), ('band', band), ('dist2', dist2)):
            if t is not None and t.device != ids_plane.device:
                raise ValueError(f'edt_band: {name} is on {t.device}, ids_plane on {ids_plane.device}')
        words = int(scratch.numel())
        return self.add(PROB_TO_ID, 4096, [0, H, W, inner, outer, limit, mid, words >> 31, words & 0x7fffffff, S], [],
                        [None, None, ids_plane, band, None, scratch, sets, dist2])

    POLY_MAX_OBJECTS = 255
    POLY_VERTEX_BLOCK = 1024  # lattice vertices per block of the edge sweeps (csrc/polygons.hip PLY_VPB)
    POLY_SLOT_BLOCK = 256     # edge slots per block of the ring-head tables (PLY_T)
    POLY_SMALL_EDGES = 4096   # up to this many boundary edges one workgroup traces in LDS (PLY_SMALL); more take the general chain

    @classmethod
    def polygon_scratch_words(cls, H, W, n, edge_capacity):
        """int32 words of the scratch of polygon_trace (csrc/polygons.hip ply_layout), with NV = (H + 1)(W + 1) lattice vertices and C =
        edge_capacity, every array rounded up to 4 words: 64 of header, a total per block of 1024 vertices, the first slot per vertex
        (NV), per edge slot its edge index, object row and predecessor (3 C), two buffers of the pointer-jumping state (2 x 5 C), the
        ring's vertex offset (C), two tables of 256 rows per block of 256 slots, and 512 row offsets.  ``n`` does not enter."""
        NV, C = (H + 1) * (W + 1), int(edge_capacity)
        up4 = lambda v: (v + 3) & ~3
        return 64 + up4(-(-NV // cls.POLY_VERTEX_BLOCK)) + up4(NV) + 14 * up4(C) + 512 * -(-C // cls.POLY_SLOT_BLOCK) + 512

    @staticmethod
    def polygon_capacity(H, W):
        """(stream bytes, edge capacity) that hold ANY plane of H x W: V <= 4 (H + 1)(W + 1) corners and R <= V / 4 rings of 16 bytes, so
        32 bytes per lattice vertex; E <= 2 (H (W + 1) + (H + 1) W), every crack in both directions."""
        return 32 * (H + 1) * (W + 1), 2 * (H * (W + 1) + (H + 1) * W)

    def polygon_trace(self, ids_plane, obj_ids, stream, table, status, scratch, *, connectivity=8, edge_capacity, path=0):
        """PROB_TO_ID flags == 8192 (ABI 11, form added; include/cutie_hip.h): ids_plane uint8 [H, W] (contiguous, any alignment, read
        only) -> the outlines of the objects of ``obj_ids`` (a sequence of ints, or an int32 tensor of them on the device, which is not
        inspected; at most 255) as rings of lattice corners.  ``stream`` (uint8 or int32, contiguous, 16-byte aligned, a multiple of 4
        bytes) receives rings int32 [R, 4] (object row | first vertex | vertices | unit edges) and directly behind them vertices uint32
        [V] (x | y << 16); ``table`` int32 [n, 4]: first ring | rings | first vertex | vertices per entry of the list; ``status`` int32
        [4]: stream bytes 16 R + 4 V | error bits (1: the stream does not fit, nothing is written to it; 2: more boundary edges than
        ``edge_capacity``, nothing is traced) | R | E.  ``scratch``: int32, 16-byte aligned, at least ``polygon_scratch_words(H, W, n,
        edge_capacity)`` words.  ``connectivity`` 8 joins diagonal pixels into one ring, 4 keeps them apart.  ``path`` 1 forces the
        general launch chain; the results are the same."""
        _need_form(_lib.has_polygons, 'no polygon trace, PROB_TO_ID flags == 8192')
        H, W = _u8_plane('polygon_trace', 'ids_plane', ids_plane)
        if H > 65535 or W > 65535:
            raise ValueError(f'polygon_trace: a plane of {H} x {W}: a vertex packs x and y into 16 bits each, H, W <= 65535')
        if (H + 1) * (W + 1) >= 1 << 29:
            raise ValueError(f'polygon_trace: a plane of {H} x {W} has 2^29 lattice vertices or more')
        n, objs, listed = _object_ids('polygon_trace', 'obj_ids', obj_ids)
        if not 0 <= n <= self.POLY_MAX_OBJECTS:
            raise ValueError(f'polygon_trace: {n} objects, 0 .. {self.POLY_MAX_OBJECTS}')
        connectivity, edge_capacity, path = int(connectivity), int(edge_capacity), int(path)
        if connectivity not in (4, 8):
            raise ValueError(f'polygon_trace: connectivity {connectivity}, 4 or 8')
        if path not in (0, 1):
            raise ValueError(f'polygon_trace: path {path}, 0 (the launcher chooses) or 1 (the general path)')
        if not 1 <= edge_capacity < 1 << 31:
            raise ValueError(f'polygon_trace: edge_capacity {edge_capacity}, 1 .. 2^31 - 1')
        if stream.dtype not in (torch.uint8, torch.int32) or not stream.is_contiguous():
            raise ValueError(f'polygon_trace: stream is a contiguous uint8 or int32 buffer, not {stream.dtype}')
        cap = int(stream.numel()) * stream.element_size()
        if cap % 4 or cap >= 1 << 31:
            raise ValueError(f'polygon_trace: a stream of {cap} bytes: a multiple of 4 below 2^31')
        if table.dtype != torch.int32 or table.numel() != n * 4 or not table.is_contiguous():
            raise ValueError(f'polygon_trace: table is a contiguous int32 [{n}, 4]')
        if status.dtype != torch.int32 or status.numel() != 4 or not status.is_contiguous():
            raise ValueError('polygon_trace: status is a contiguous int32 [4]')
        need = self.polygon_scratch_words(H, W, n, edge_capacity)
        if scratch.dtype != torch.int32 or not scratch.is_contiguous() or scratch.numel() < need:
            raise ValueError(f'polygon_trace: scratch is a contiguous int32 of at least {need} words')
        for name, t in (('stream', stream), ('scratch', scratch)) + ((('table', table),) if n else ()):
            if t.data_ptr() % 16:
                raise ValueError(f'polygon_trace: {name} is 16-byte aligned')
        for name, t in (('stream', stream), ('table', table), ('status', status), ('scratch', scratch)):
            if t.device != ids_plane.device:
                raise ValueError(f'polygon_trace: {name} is on {t.device}, ids_plane on {ids_plane.device}')
        if objs is None and n:
            objs = torch.tensor(listed, dtype=torch.int32).to(ids_plane.device)
            self.keep.append(objs)
        words = int(scratch.numel())
        return self.add(PROB_TO_ID, 8192, [0, H, W, edge_capacity, cap, connectivity, path, words >> 31, words & 0x7fffffff, n], [],
                        [None, None, ids_plane, stream, status, scratch, objs if n else None, table if n else None])

    JPEG_ENC_BLOCK_WORDS = 52     # JPG_BLOCK_WORDS (csrc/jpeg_enc.hip): a coded block is at most 22 + 63 * 26 = 1660 bits

    @staticmethod
    def jpeg_enc_blocks(H, W):
        """Coded blocks of a 4:2:0 frame: six (Y00 Y01 Y10 Y11 Cb Cr) per 16 x 16 MCU."""
        return 6 * -(-H // 16) * -(-W // 16)

    @classmethod
    def jpeg_enc_scratch_words(cls, H, W):
        """int32 words of the scratch of jpeg_encode (csrc/jpeg_enc.hip jpg_scratch_words; include/cutie_hip.h ABI 11): 16 words of
        header, per coded block 32 words of coefficients, 4 of offsets and bit counts and 52 of the unstuffed stream (+ 16), and 4 words
        per 16-word chunk of that stream."""
        B = cls.jpeg_enc_blocks(H, W)
        U = cls.JPEG_ENC_BLOCK_WORDS * B + 16
        return 16 + 32 * B + 4 * B + U + 4 * -(-U // 16)

    @classmethod
    def jpeg_enc_capacity(cls, H, W, worst=False):
        """Bytes of the stream buffer of jpeg_encode.  worst=True: what holds the segment of ANY frame -- every coded block at its 1660
        bits and every byte a stuffed 0xFF: 2 * ceil(1660 blocks / 8) bytes, ~10 bytes per pixel, which no picture comes near.  The
        default is the practical size the saver allocates: 1024 + 1.5 bytes per pixel, capped by the worst case (quality-75 overlays of
        video frames take 0.05 .. 0.3 bytes per pixel, uniform noise 0.6); a frame that needs more sets the overflow bit and says what
        it needs."""
        full = 2 * -(-1660 * cls.jpeg_enc_blocks(H, W) // 8)
        return full if worst else min(full, -(-(1024 + 3 * H * W // 2) // 4) * 4)

    def jpeg_encode(self, frame, ids, colors, qtables, stream, status, scratch, *, H, W, ldrow=None):
        """PROB_TO_ID flags == 128 (ABI 11, include/cutie_hip.h): frame uint8 [H, W, 3] (row stride ``ldrow`` bytes, default the
        tensor's; pixels packed) with the colours of ``colors`` (uint8 [256, 4]) blended over it where ``ids`` (uint8 [H, W] contiguous,
        or None: the frame as it is) is not 0 -> ``stream`` uint8 [capacity] = the entropy-coded segment of the baseline 4:2:0 JPEG
        that libjpeg-turbo writes for the blended frame with the quantisation tables ``qtables`` (uint16 [2, 64], natural order, 1 .. 255).
        status int32 [4] = (stream bytes, 0, error bits: 1 = the capacity is too small and nothing was written, 0); scratch int32
        [>= jpeg_enc_scratch_words(H, W)], 16-byte aligned.  inference/utils/jpeg_writer.py wraps the stream into a file."""
        H, W = int(H), int(W)
        if frame.dtype != torch.uint8 or frame.dim() != 3 or tuple(frame.shape) != (H, W, 3) or frame.stride(2) != 1 or frame.stride(1) != 3:
            raise ValueError(f'jpeg_encode: frame is uint8 [{H}, {W}, 3] with packed pixels, not {frame.dtype} {tuple(frame.shape)} strides {frame.stride()}')
        ldrow = int(frame.stride(0) if ldrow is None else ldrow)
        if ids is not None:
            if ids.dtype != torch.uint8 or tuple(ids.shape) != (H, W) or not ids.is_contiguous():
                raise ValueError(f'jpeg_encode: ids is a contiguous uint8 [{H}, {W}]')
            if colors is None or colors.dtype != torch.uint8 or colors.numel() != 1024 or not colors.is_contiguous():
                raise ValueError('jpeg_encode: colors is a contiguous uint8 [256, 4]')
        if qtables.dtype not in (torch.uint16, torch.int16) or qtables.numel() != 128 or not qtables.is_contiguous():
            raise ValueError('jpeg_encode: qtables is a contiguous 16-bit [2, 64]')
        return self.add(PROB_TO_ID, 128, [0, H, W, 0, ldrow, 0, 0, stream.numel(), min(scratch.numel(), (1 << 31) - 1)], [],
                        [frame, None, ids, stream, status, scratch, colors if ids is not None else None, qtables])

    MATTE_MODES = {'davis': 0, 'light': 1, 'fade': 2, 'popup': 3, 'layer': 4, 'alpha': 5}    # i8 of PROB_TO_ID flags == 256 (csrc/matte.hip)
    MATTE_MAX_TARGETS = 255

    @staticmethod
    def _matte_planes(who, planes):
        if planes.dim() != 3 or planes.dtype != torch.float32 or planes.stride(2) != 1 or min(planes.shape) < 1:
            raise ValueError(f'{who}: planes are f32 [P, h, w] with a contiguous last dimension, not {planes.dtype} {tuple(planes.shape)} strides {planes.stride()}')
        if max(planes.stride(0), planes.stride(1)) >= 1 << 31:
            raise ValueError(f'{who}: strides are 32-bit')
        return [int(planes.shape[0]), int(planes.shape[1]), int(planes.shape[2]), int(planes.stride(0)), int(planes.stride(1))]

    def matte_composite(self, mode, out, *, out_hw, frame=None, planes=None, targets=(), ids=None, colors=None, layer=None, matte=None, ldrow=None):
        """PROB_TO_ID flags == 256 (ABI 11, forms added, include/cutie_hip.h): one visualisation mode of the reference's interactive tool
        (gui/interactive_utils.py:152-229) -> ``out`` uint8 [OH, OW, 3] packed and contiguous, 16-byte aligned, composed in float32 in the
        reference's operation order and quantised as ``(x * 255).byte()``: the reference's bytes.  ``frame`` uint8 [OH, OW, 3] (row stride
        ``ldrow`` bytes, default the tensor's; pixels packed, any alignment).
        Hard modes 'davis' | 'light' | 'fade': ``ids`` uint8 [OH, OW] contiguous and ``colors`` uint8 [256, 4] (R, G, B, unused) -- the
        colour of every id is blended over the frame (alpha 0.5, 0.9, 0.5), 'fade' darkens the background to 0.6.
        Soft modes 'popup' | 'layer': ``planes`` f32 [P, h, w] (any plane / row strides: the view ``step`` returns is read in place;
        resampled bilinearly to (OH, OW) inside the launch exactly as prob_to_id(out_hw=...) samples them) and ``targets``, the plane
        indices whose sum -- in list order -- is the matte m: 'popup' keeps the targets in colour over a grey background, 'layer' puts
        ``layer`` (uint8 [OH, OW, 4] RGBA contiguous, 16-byte aligned) between the background and the targets.  ``matte`` (optional,
        soft modes): uint8 [OH, OW] contiguous, 16-byte aligned = clamp(m, 0, 1) quantised -- the fourth channel of the reference's
        'rgba' mode; mode 'alpha' writes the matte alone (``out``, ``frame`` unused, may be None).
        The target list is read by the launcher when the list runs (it checks every index); it is kept alive here."""
        code = self.MATTE_MODES.get(mode)
        if code is None:
            raise ValueError(f'matte_composite: mode is one of {tuple(self.MATTE_MODES)}, not {mode!r}')
        OH, OW = int(out_hw[0]), int(out_hw[1])
        soft = code >= 3
        ints = [0] * 10
        ints[5], ints[6], ints[8] = OH, OW, code
        tg = None
        if soft:
            if planes is None:
                raise ValueError(f'matte_composite: mode {mode!r} needs planes')
            ints[:5] = self._matte_planes('matte_composite', planes)
            tg = np.array([int(q) for q in targets], dtype=np.int32)
            if len(tg) > self.MATTE_MAX_TARGETS or (len(tg) and (tg.min() < 0 or tg.max() >= ints[0])):
                raise ValueError(f'matte_composite: at most {self.MATTE_MAX_TARGETS} targets, each a plane index 0 .. {ints[0] - 1}, not {tg.tolist()}')
            ints[9] = len(tg)
            self.keep.append(tg)
            if matte is not None and (matte.dtype != torch.uint8 or tuple(matte.shape) != (OH, OW) or not matte.is_contiguous()):
                raise ValueError(f'matte_composite: matte is a contiguous uint8 [{OH}, {OW}]')
            if code == 5 and matte is None:
                raise ValueError("matte_composite: mode 'alpha' needs matte")
        elif matte is not None:
            raise ValueError(f'matte_composite: mode {mode!r} has no matte (popup, layer, alpha)')
        if code != 5:
            if frame is None or frame.dtype != torch.uint8 or tuple(frame.shape) != (OH, OW, 3) or frame.stride(2) != 1 or frame.stride(1) != 3:
                raise ValueError(f'matte_composite: frame is uint8 [{OH}, {OW}, 3] with packed pixels')
            if out is None or out.dtype != torch.uint8 or tuple(out.shape) != (OH, OW, 3) or not out.is_contiguous():
                raise ValueError(f'matte_composite: out is a contiguous uint8 [{OH}, {OW}, 3]')
            ints[7] = int(frame.stride(0) if ldrow is None else ldrow)
            if not soft:
                if ids is None or ids.dtype != torch.uint8 or tuple(ids.shape) != (OH, OW) or not ids.is_contiguous():
                    raise ValueError(f'matte_composite: mode {mode!r} needs ids, a contiguous uint8 [{OH}, {OW}]')
                if colors is None or colors.dtype != torch.uint8 or colors.numel() != 1024 or not colors.is_contiguous():
                    raise ValueError('matte_composite: colors is a contiguous uint8 [256, 4]')
            if code == 4 and (layer is None or layer.dtype != torch.uint8 or tuple(layer.shape) != (OH, OW, 4) or not layer.is_contiguous()):
                raise ValueError(f'matte_composite: mode layer needs layer, a contiguous uint8 [{OH}, {OW}, 4]')
        else:
            frame = out = None
        return self.add(PROB_TO_ID, 256, ints, [],
                        [planes if soft else None, int(tg.ctypes.data) if (tg is not None and len(tg)) else None, frame, out, matte,
                         None if soft else ids, None if soft else colors, layer if code == 4 else None])

    def matte_soft(self, planes, out, *, out_hw):
        """PROB_TO_ID flags == 512 (ABI 11, forms added, include/cutie_hip.h): the soft masks of the reference's interactive tool
        (gui/resource_manager.py:166-173) -- ``planes`` f32 [P, h, w] (strides as in matte_composite), every object plane q >= 1 sampled at
        (OH, OW) as prob_to_id(out_hw=...) samples it and quantised as ``(p * 255).astype(uint8)`` -> ``out`` uint8 [P - 1, OH, OW]
        contiguous, 16-byte aligned.  P == 1 writes nothing."""
        OH, OW = int(out_hw[0]), int(out_hw[1])
        ints = self._matte_planes('matte_soft', planes) + [OH, OW]
        if out.dtype != torch.uint8 or tuple(out.shape) != (ints[0] - 1, OH, OW) or not out.is_contiguous():
            raise ValueError(f'matte_soft: out is a contiguous uint8 [{ints[0] - 1}, {OH}, {OW}]')
        return self.add(PROB_TO_ID, 512, ints, [], [planes, None, out])

    def resize(self, src, dst, *, C, H, W, OH, OW, plane, ldrow, nearest=False, antialias=False, src_u8=False, taps=None, scratch=None):
        """RESIZE.  antialias: F.interpolate(bilinear, antialias=True) -- taps = resize_aa_table(H, W, OH, OW) on the device (int32
        [OW + OH, K + 2]), scratch = f32 [C, H, OW].  src_u8: src is u8 [H, W, C] with row stride `ldrow` bytes (ToTensor on the fly;
        without antialias OH == H, OW == W).  include/cutie_hip.h (ABI 5)."""
        if nearest and (antialias or src_u8):
            raise ValueError('resize: nearest excludes antialias / src_u8')
        flags = (1 if nearest else 0) | (2 if antialias else 0) | (4 if src_u8 else 0)
        ints = [C, H, W, OH, OW, plane, ldrow]
        ptrs = [src, dst]
        if antialias:
            if taps is None or scratch is None:
                raise ValueError('resize(antialias=True) needs taps= and scratch=')
            ints.append(taps.shape[1] - 2)
            ptrs += [taps, scratch]
        return self.add(RESIZE, flags, ints, [], ptrs)

    def _jpeg(self, flag, pkt, *, work=None, coef=None, status=None, planes=None, rgb=None, rounds=JPEG_SYNC_ROUNDS):
        """RESIZE flags 8 / 16 / 32 (include/cutie_hip.h, ABI 6): one stage of the JPEG decode of `pkt` (inference/data/jpeg.py
        Packet; its uint8 buffer on the device is `pkt_dev`) -- the geometry comes from the packet header."""
        from .inference.data import jpeg as J
        host, dev = pkt
        h = host.hdr
        ints = [h[J.HDR_NCHUNK], h[J.HDR_NSEG], h[J.HDR_NBLOCK], h[J.HDR_CHUNK_BITS], rounds, host.buf.nbytes, h[J.HDR_PLANE_BYTES],
                h[J.HDR_H], h[J.HDR_W], 0 if work is None else work.numel(), h[J.HDR_NCOMP], 3 * int(h[J.HDR_W])]
        return self.add(RESIZE, flag, ints, [], [dev, work, coef, status, planes, rgb])

    def jpeg_huff(self, pkt, *, work, coef, status, rounds=JPEG_SYNC_ROUNDS):
        """Stage 1: entropy decode -> coef int16 [nblock, 64] (natural order, quantised, absolute DC).  pkt = (Packet, device uint8
        copy of Packet.buf); work int32 >= jpeg.work_words(...), status int32 [4] (error bits, sync rounds, serial segments)."""
        return self._jpeg(8, pkt, work=work, coef=coef, status=status, rounds=rounds)

    def jpeg_idct(self, pkt, *, coef, planes):
        """Stage 2: ISLOW IDCT -> planes uint8 (every component, whole blocks)."""
        return self._jpeg(16, pkt, coef=coef, planes=planes)

    def jpeg_color(self, pkt, *, planes, rgb):
        """Stage 3: fancy upsampling + YCbCr -> RGB -> rgb uint8 [H, W, 3] packed."""
        return self._jpeg(32, pkt, planes=planes, rgb=rgb)

    @staticmethod
    def jpeg_layout(packets, rounds=JPEG_SYNC_ROUNDS, guard=0):
        """The buffers of one batch JPEG decode over ``packets`` (inference/data/jpeg.py Packet) -> (table int32 [N, 8], sizes).  Table row
        (include/cutie_hip.h, ABI 11, forms added): the offsets of the image's packet (bytes, a multiple of 16), work area (int32 words, 8-byte
        aligned), coefficients (int16 elements, 16-byte aligned), planes (bytes, 8-byte aligned) and rgb (bytes, 16-byte aligned), its
        packet bytes, its rgb row stride (3 W), 0.  ``sizes``: the element counts of the buffers -- 'packets' uint8, 'work' int32, 'coef'
        int16, 'planes' uint8, 'rgb' uint8 (per image jpeg.stage_sizes, rounded up to the alignment) -- the largest 'max_chunk' /
        'max_seg' / 'max_block' / 'max_pix' of the batch (the grids) and 'rounds'.  ``guard`` bytes (a multiple of 16) lie in front of
        and behind every image's region in coef, planes and rgb.  Every buffer stays below 2^31 bytes (ValueError)."""
        from .inference.data import jpeg as J
        if guard < 0 or guard % 16:
            raise ValueError('jpeg batch: guard is a multiple of 16 bytes')
        table = np.zeros((len(packets), 8), dtype=np.int32)
        po = wo = co = plo = ro = 0
        mx = [0, 0, 0, 0]
        for k, pkt in enumerate(packets):
            sz, h = J.stage_sizes(pkt, rounds), pkt.hdr
            co += guard // 2
            plo += guard
            ro += guard
            W = int(h[J.HDR_W])
            row = (po, wo, co, plo, ro, pkt.buf.nbytes, 3 * W, 0)
            po += -(-pkt.buf.nbytes // 16) * 16
            wo += -(-sz['work'] // 2) * 2
            co += -(-(sz['coef'] + guard // 2) // 8) * 8
            plo += -(-(sz['planes'] + guard) // 8) * 8
            ro += -(-(sz['rgb'] + guard) // 16) * 16
            if max(po, 4 * wo, 2 * co, plo, ro) >= 1 << 31:
                raise ValueError('jpeg batch: the buffers of one launch stay below 2^31 bytes')
            table[k] = row
            mx = [max(a, int(b)) for a, b in zip(mx, (h[J.HDR_NCHUNK], h[J.HDR_NSEG], h[J.HDR_NBLOCK], int(h[J.HDR_H]) * W))]
        return table, {'packets': po, 'work': wo, 'coef': co, 'planes': plo, 'rgb': ro, 'rounds': rounds,
                       'max_chunk': mx[0], 'max_seg': mx[1], 'max_block': mx[2], 'max_pix': mx[3]}

    def _jpeg_batch(self, flags, packets, table, sizes, status, *, n, work=None, coef=None, planes=None, rgb=None):
        """RESIZE flags 8 / 16 / 32 with 256 (include/cutie_hip.h, ABI 11, forms added): one stage of the JPEG decode of ``n`` packets in the
        uint8 buffer ``packets``, laid out by ``table`` / ``sizes`` (jpeg_layout); every stage gets the same table, sizes and status."""
        # as _png: the forms came without a new ABI number, and a library from before would read the descriptor as a one-frame decode
        if not getattr(_lib._executor, 'is_mock', False):
            try:
                known = _lib.has_jpeg_batch()
            except _lib.HipLibraryError:
                known = True
            if not known:
                raise _lib.HipLibraryError(f'{_lib.LIB_PATH} is stale (no batch JPEG decode, RESIZE flags 256); rebuild it.')
        if not 1 <= n <= 65535:
            raise ValueError(f'jpeg batch: {n} images, 1 .. 65535')
        if table.dtype != torch.int32 or table.numel() < 8 * n or not table.is_contiguous():
            raise ValueError(f'jpeg batch: table is a contiguous int32 [{n}, 8]')
        if status.dtype != torch.int32 or status.numel() < 4 * n or not status.is_contiguous():
            raise ValueError(f'jpeg batch: status is a contiguous int32 [{n}, 4]')
        for name, t, dt in (('packets', packets, torch.uint8), ('work', work, torch.int32), ('coef', coef, torch.int16),
                            ('planes', planes, torch.uint8), ('rgb', rgb, torch.uint8)):
            if t is not None and (t.dtype != dt or not t.is_contiguous() or t.numel() < sizes[name]):
                raise ValueError(f'jpeg batch: {name} is a contiguous {dt} buffer of at least {sizes[name]} elements')
        ints = [n] + [sizes[k] for k in ('packets', 'work', 'coef', 'planes', 'rgb', 'rounds', 'max_chunk', 'max_seg', 'max_block', 'max_pix')]
        return self.add(RESIZE, flags | 256, ints, [], [packets, table, work, coef, planes, rgb, status])

    def jpeg_huff_batch(self, packets, table, sizes, status, *, n, work, coef):
        """Stage 1 over ``n`` images, one launch per pass: -> coef int16 (per image [nblock, 64] at its table offset), status int32 [n, 4],
        cleared by the launch: per image error bits (1 bad code, 2 data ends early, 4 bad table or header: the image is skipped), sync
        rounds, serial segments.  work int32, 8-byte aligned; coef 16-byte aligned."""
        return self._jpeg_batch(8, packets, table, sizes, status, n=n, work=work, coef=coef)

    def jpeg_idct_batch(self, packets, table, sizes, status, *, n, coef, planes):
        """Stage 2 over ``n`` images in one launch: -> planes uint8 (per image at its table offset)."""
        return self._jpeg_batch(16, packets, table, sizes, status, n=n, coef=coef, planes=planes)

    def jpeg_color_batch(self, packets, table, sizes, status, *, n, planes, rgb):
        """Stage 3 over ``n`` images in one launch: -> rgb uint8 (per image [H, W, 3] packed at its table offset)."""
        return self._jpeg_batch(32, packets, table, sizes, status, n=n, planes=planes, rgb=rgb)

    @staticmethod
    def png_layout(packets, guard=0):
        """The buffers of one PNG decode launch over ``packets`` (inference/data/png_packet.py Packet) -> (table int32 [N, 4] = per image the
        byte offset of its packet, of its inflated rows and of its pixels, 0; packet bytes, inflate bytes, output bytes).  Packets and
        inflated rows start at multiples of 16; pixels at multiples of 16 too, with ``guard`` bytes in front of and behind every image."""
        table = np.zeros((len(packets), 4), dtype=np.int32)
        po = io = oo = 0
        for k, pkt in enumerate(packets):
            oo += guard
            table[k, :3] = po, io, oo
            po += -(-pkt.buf.nbytes // 16) * 16
            io += -(-pkt.inflated // 16) * 16
            oo += -(-(pkt.nbytes_out + guard) // 16) * 16
            if max(po, io, oo) >= 1 << 31:
                raise ValueError('png decode: the buffers of one launch stay below 2^31 bytes')
        return table, po, io, oo

    def _png(self, flags, packets, table, inflate, out, status, *, n, packet_bytes=None):
        # the forms came without a new ABI number: a library from before would run the descriptor as a plain RESIZE, so ask it first
        # (an injected interpreter of the tests has no library; a missing library fails when the list runs)
        if not getattr(_lib._executor, 'is_mock', False):
            try:
                known = _lib.has_png_decode()
            except _lib.HipLibraryError:
                known = True
            if not known:
                raise _lib.HipLibraryError(f'{_lib.LIB_PATH} is stale (no PNG decode stages, RESIZE flags 64 / 128); rebuild it.')
        if table.dtype != torch.int32 or table.numel() < 4 * n or status.dtype != torch.int32 or status.numel() < 4 * n:
            raise ValueError(f'png decode: table and status are int32 [{n}, 4]')
        for name, t in (('packets', packets), ('inflate', inflate)) + ((('out', out),) if out is not None else ()):
            if t.dtype != torch.uint8 or not t.is_contiguous():
                raise ValueError(f'png decode: {name} is a contiguous uint8 buffer')
        if not 1 <= n <= 65535:
            raise ValueError(f'png decode: {n} images, 1 .. 65535')
        return self.add(RESIZE, flags, [n, packets.numel() if packet_bytes is None else packet_bytes, inflate.numel(), 0 if out is None else out.numel()], [],
                        [packets, table, inflate, out, status])

    def png_inflate(self, packets, table, inflate, status, *, n, packet_bytes=None):
        """RESIZE flags 64 (ABI 11, forms added, include/cutie_hip.h): the zlib streams of ``n`` PNG packets (uint8 buffer ``packets``, laid out by
        ``table`` int32 [n, 4] -- png_layout) inflated into ``inflate`` (uint8, the filtered rows), one wave per image.  ``status`` int32
        [n, 4], cleared by the launch: error bits, bytes produced, blocks, tokens.  All buffers 16-byte aligned."""
        return self._png(64, packets, table, inflate, None, status, n=n, packet_bytes=packet_bytes)

    def png_unfilter(self, packets, table, inflate, out, status, *, n, packet_bytes=None):
        """RESIZE flags 128 (ABI 11, forms added): the filtered rows of png_inflate -> ``out`` uint8: per image [H, W] (palette index or grey value,
        pixels of 1 / 2 / 4 bits unpacked) or [H, W, 3] at its table offset.  An image whose status has an error bit is left alone; a
        filter byte above 4 sets one."""
        return self._png(128, packets, table, inflate, out, status, n=n, packet_bytes=packet_bytes)

    def flip_w(self, src, dst, *, rows, W, slds=None, dlds=None, alpha=1.0, beta=0.0):
        return self.add(FLIP_W, 0, [rows, W, W if slds is None else slds, W if dlds is None else dlds], [alpha, beta], [src, dst])

    def cast(self, src, dst, *, n, to_f32=False):
        return self.add(CAST, 1 if to_f32 else 0, [n], [], [src, dst])
