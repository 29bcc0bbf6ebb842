"""The filtered, dynamic-Huffman PNG stage without a GPU: the model of the kernels (tests/png_photo_ref.py) against zlib, PIL and the
project's own inflater on the whole corpus (tests/png_photo_corpus.py); the code builder function by function; the sizes against the
fixed form and against PIL; the reference's recorded 'rgba' bytes through matte model, encoder and PIL; the descriptor; and the saver and
the parser through the descriptor interpreter (tests/mock_exec_png_photo.py)."""
import io
import glob
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from cutie_amd import _lib, ops as O
from cutie_amd.inference.utils import png as PNG
from cutie_amd.inference.utils import results_utils as RU

import matte_ref as M
import png_dec_ref as D
import png_photo_corpus as C
import png_photo_ref as P
import png_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, 'golden', 'matte', '*.npz')))
# the model's worst file size against PIL's default save of the same pixels, computed on this corpus (profiles/png_photo.md); + 0.05 for
# other zlib builds
PHOTO_WORST, SMOOTH_WORST = 1.046, 1.845


def _file(name):
    e = C.encoded(name)
    return PNG.assemble_image(e['stream'], e['H'], (e['L'] - 1) // e['B'], e['B'])


def _pixels(name):
    s0, s1 = C.corpus()[name]
    raw, B = P.raw_rows(s0, s1)
    return raw.reshape(raw.shape[0], -1, B).squeeze(-1) if B == 1 else raw.reshape(raw.shape[0], -1, B)


def _pil_bytes(px):
    b = io.BytesIO()
    Image.fromarray(px).save(b, 'PNG')
    return len(b.getvalue())


# ---- the model on the corpus ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(C.corpus()))
def test_model_stream_inflates_and_opens(name):
    s0, s1 = C.corpus()[name]
    e = C.encoded(name)
    H, L, B = e['H'], e['L'], e['B']
    W = (L - 1) // B
    assert zlib.decompress(e['stream']) == e['filtered'].tobytes()
    P.check_stream(e['stream'], e['filtered'])
    assert len(e['stream']) == e['size'] <= P.capacity(H, L) == O.OpList.png_photo_capacity(H, W, B)
    assert P.scratch_words(H, L) == O.OpList.png_photo_scratch_words(H, W, B)
    im = Image.open(io.BytesIO(_file(name)))
    im.load()
    assert im.mode == P.MODE[B] and im.size == (W, H)
    assert np.array_equal(np.array(im), _pixels(name))
    if s1 is None:                                                               # the project's own inflater: L and RGB
        from cutie_amd.inference.data import png_packet
        pk, why = png_packet.parse(_file(name), name)
        assert pk is not None, why
        got, st = D.decode(pk)
        assert st[0] == 0 and np.array_equal(got, _pixels(name))


def test_corpus_covers_what_it_must():
    items = C.corpus()
    enc = {k: C.encoded(k) for k in items}
    wins = set()
    for k in C.ramps():
        wins |= set(enc[k]['filters'].tolist())
    assert wins == {0, 1, 2, 3, 4}                                               # each of the five filters wins a row of the ramps
    assert int((enc['ramp_up']['filters'] == 2).sum()) > 12 and int((enc['ramp_none']['filters'] == 0).sum()) > 12
    shapes = {(e['H'], e['L'], e['B']) for e in enc.values()}
    assert {(1, 2, 1), (1, 3, 1), (2, 2, 1), (1, 5, 4)} <= shapes
    assert {L for _, L, B in shapes if B == 1} >= {63, 64, 65, 128, 129, P.ROW_LIMIT}
    assert {L for _, L, B in shapes if B == 4} >= {61, 65, 125, 129, 4 * 4095 + 1}
    assert {H for H, _, _ in shapes} >= {P.R - 1, P.R, P.R + 1, 2 * P.R + 1}
    assert {e['B'] for e in enc.values()} == {1, 2, 3, 4}
    forms = {f for e in enc.values() for f in e['forms']}
    assert forms == {'fixed', 'dynamic'}
    assert enc['1x1']['forms'] == ['fixed'] and len(enc['1x1']['stream']) == 10  # a tiny image pays for no header
    # no match at all / every match at one distance / the take rule's lengths
    kinds = lambda e: np.concatenate([t[1] for t in e['tokens']])
    lens = lambda e: np.concatenate([t[2][t[1] >= 0] for t in e['tokens']])
    assert (kinds(enc['noise']) < 0).all() and (kinds(enc['fib']) < 0).all()
    assert set(kinds(enc['1xW'])[kinds(enc['1xW']) >= 0].tolist()) == {0}
    assert {0, 2} <= set(kinds(enc['blocks']).tolist())
    for name in ('period_rgba', 'period_rgb', 'period_la'):                      # matches at distance B, for B = 4, 3, 2
        assert 1 in set(kinds(enc[name]).tolist()), name
    seen = set()
    for n in (257, 258, 259, 260, 261, 262, 263, 516, 517, 518, 519, 520):
        seen |= set(lens(enc[f'run{n}']).tolist()) | set(lens(enc[f'run{n}_edge']).tolist())
    assert {256, 257, 258} <= seen and max(seen) == 258 and min(seen) >= P.MINMATCH
    for e in enc.values():                                                       # tokens tile every row, matches are >= MINMATCH
        for st, kd, ln in e['tokens']:
            assert st[0] == 0 and np.array_equal(st[1:], (st + ln)[:-1]) and st[-1] + ln[-1] == e['L']
            assert (ln[kd >= 0] >= P.MINMATCH).all() and (ln[kd < 0] == 1).all()


def test_fibonacci_counts_need_the_length_limit():
    e = C.encoded('fib')
    assert e['forms'] == ['dynamic'] and (e['filters'] == 0).all()
    ll = np.bincount(e['filtered'].ravel(), minlength=286)
    ll[256] = 1
    assert P.code_lengths(ll, 40).max() > 15 and P.code_lengths(ll, 15).max() == 15


def test_capacity_error_is_modelled():
    s0, s1 = C.corpus()['bike_rgba']
    need = C.encoded('bike_rgba')['size']
    for cap in (0, 3, need - 1, (need + 3) // 4 * 4 - 4):
        stream, status = P.stage(s0, s1, cap)
        assert stream is None and status.tolist()[0] == need and status[2] == 1 and status[3] == 0
    stream, status = P.stage(s0, s1, (need + 3) // 4 * 4)
    assert stream == C.encoded('bike_rgba')['stream'] and status[2] == 0
    assert int(status[1]) & 0xffffffff == zlib.adler32(C.encoded('bike_rgba')['filtered'].tobytes()) & 0xffffffff


# ---- the code builder --------------------------------------------------------------------------------------------------------------------
def _kraft(lengths, limit):
    return sum(1 << (limit - int(l)) for l in lengths if l)


def test_code_lengths_are_complete_and_limited():
    rng = np.random.default_rng(3)
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    cases = [fib[:n] for n in (2, 3, 8, 9, 10, 16, 17, 19, 25, 30)] + [[1] * n for n in (2, 3, 5, 19, 30, 286)]
    cases += [rng.integers(0, 50, n).tolist() for n in (19, 30, 286) for _ in range(5)]
    cases += [(rng.integers(0, 3, 286) * rng.integers(1, 100000, 286)).tolist() for _ in range(5)]
    for counts in cases:
        for limit in (7, 15):
            n = sum(1 for c in counts if c > 0)
            if n < 2 or n > 1 << limit:
                continue
            lens = P.code_lengths(counts, limit)
            assert ((lens > 0) == (np.array(counts) > 0)).all() and lens.max() <= limit
            assert _kraft(lens, limit) == 1 << limit                             # the Kraft sum is exactly 1
            act = [s for s in range(len(counts)) if counts[s]]
            assert all(lens[a] >= lens[b] for a in act for b in act if counts[a] < counts[b])    # a rarer symbol is never shorter
            codes = P.canonical(lens)
            words = sorted(format(int(codes[s]), f'0{int(lens[s])}b')[::-1] for s in act)
            assert all(not b.startswith(a) for a, b in zip(words, words[1:]))    # prefix-free
    # the limiter alone, on the alphabet it serves: 19 Fibonacci counts would be 18 deep
    assert P.code_lengths(fib[:19], 40).max() == 18 and P.code_lengths(fib[:19], 7).max() == 7
    assert _kraft(P.code_lengths(fib[:19], 7), 7) == 128
    # an unlimited code is Huffman's: its cost equals heapq's
    import heapq
    for counts in cases[-10:]:
        h = [c for c in counts if c > 0]
        heapq.heapify(h)
        cost = 0
        while len(h) > 1:
            a, b = heapq.heappop(h), heapq.heappop(h)
            cost += a + b
            heapq.heappush(h, a + b)
        assert int((P.code_lengths(counts, 40) * np.array(counts)).sum()) == cost


def test_degenerate_alphabets():
    assert P.code_lengths([0] * 30, 15).tolist() == [0] * 30                     # no match: no distance code
    one = P.code_lengths([0, 0, 7] + [0] * 27, 15)
    assert one.tolist() == [0, 0, 1] + [0] * 27 and P.canonical(one)[2] == 0      # one distance symbol: one bit, one unused code
    for name, ndist in (('noise', 0), ('1xW', 1)):
        e = C.encoded(name)
        assert 'dynamic' in e['forms']
        assert zlib.decompress(e['stream']) == e['filtered'].tobytes()           # zlib's inflate accepts both
    hdr, (hlit, hdist, hclen, cl) = P.dynamic_header(P.code_lengths([3, 1] + [0] * 254 + [1] + [0] * 29, 15), np.zeros(30, np.int64), True)
    assert (hlit, hdist) == (257, 1) and 4 <= hclen <= 19 and cl.max() <= 7 and hdr[0] == (5, 3)
    # the greedy rule: 138 zeros, 12 zeros, a 3, six more 3s, two 3s one by one, four zeros, three 5s one by one
    assert P.rle_lengths([0] * 150 + [3] * 9 + [0] * 4 + [5, 5, 5]) == [(18, 7, 127), (18, 7, 1), (3, 0, 0), (16, 2, 3), (3, 0, 0), (3, 0, 0), (17, 3, 1),
                                                                        (5, 0, 0), (5, 0, 0), (5, 0, 0)]


def test_code_length_code_limit_search():
    """No seeded plane of 64 x 256 or below was found whose code-length code passes 7 bits before limiting (C.CL_SEED is None; DESIGN.md
    section 24): the function-level check above covers the model's limiter, and test_encoder_core_under_sanitizers below executes the
    shipped one (csrc/deflate_enc_core.h) at limit 7 on the host, from count vectors.  Should a seed be committed, its plane must need
    the limit."""
    if C.CL_SEED is not None:
        e = P.encode(C.cl_candidate(C.CL_SEED))
        assert zlib.decompress(e['stream']) == e['filtered'].tobytes()


# ---- the shipped code builder on the host ---------------------------------------------------------------------------------------------
CL_DEEP_SEEDS = (0, 2, 3)          # _split_counts(seed): literal/length counts whose code-length code is 8 deep before limiting


def _host_compiler():
    for cc in (os.environ.get('CXX'), 'c++', 'g++', 'clang++'):
        if cc and shutil.which(cc):
            return shutil.which(cc)
    return None


def _split_counts(seed):
    """A complete prefix code grown by splitting leaves (a random one or the deepest, by a coin), every symbol counted 2^(15 - length) so
    that Huffman gives those lengths back: many lengths with skewed frequencies of their own, which is what deepens the code-length code."""
    rng = np.random.default_rng(seed)
    leaves, n = [0], int(rng.integers(20, 287))
    while len(leaves) < n:
        ok = [k for k, d in enumerate(leaves) if d < 15]
        k = ok[int(rng.integers(len(ok)))] if rng.random() < 0.5 else max(ok, key=lambda k: leaves[k])
        d = leaves.pop(k)
        leaves += [d + 1, d + 1]
    ll = np.zeros(286, np.int64)
    ll[rng.permutation(286)[:n]] = [1 << (15 - d) for d in leaves]
    return ll


def _cl_counts(ll_len, d_len):
    _, (hlit, hdist, _, _) = P.dynamic_header(ll_len, d_len, True)
    cl_cnt = np.zeros(19, np.int64)
    for s, _, _ in P.rle_lengths(list(ll_len[:hlit]) + list(d_len[:hdist])):
        cl_cnt[s] += 1
    return cl_cnt


def _random_counts(rng, kind, n):
    if kind == 'uniform':
        return rng.integers(0, 50, n)
    if kind == 'sparse':
        return rng.integers(0, 3, n) // 2 * rng.integers(1, 100000, n)
    if kind == 'fibonacci':                                                      # a + b of the two before, jittered, in a random order
        v = [1, 1]
        while len(v) < min(n, 40):
            v.append(v[-1] + v[-2] + int(rng.integers(0, 2)))
        out = np.zeros(n, np.int64)
        out[rng.permutation(n)[:len(v)]] = v
        return out
    return rng.permutation((1 << np.minimum(np.arange(n), 20) // int(rng.integers(1, 4))).astype(np.int64))    # geometric


def test_encoder_core_under_sanitizers(tmp_path):
    """png_enc_host.cpp = the encoders' scalar core (csrc/deflate_enc_core.h) with its own main, built with -fsanitize=address,undefined,
    every work array a heap block of the kernel's size: the counts of every block of the corpus, the degenerate alphabets, count vectors
    that need the limiter at 15 and at 7 (the code-length code's: seeded vectors, asserted to need it) and every length and distance go
    through it on the CPU; its lengths, codes and header bytes equal the model's."""
    cc = _host_compiler()
    if cc is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'png_enc_host')
    subprocess.run([cc, '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    os.path.join(HERE, '..', 'cutie_amd', 'csrc', 'png_enc_host.cpp'), '-o', exe], check=True)
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    none = np.zeros(30, np.int64)
    eob = np.zeros(286, np.int64)
    eob[256] = 1
    two = eob.copy()
    two[65] = 9
    blocks = [(name, ll, dd, final) for name in C.corpus() for ll, dd, final in P.band_counts(C.encoded(name))]
    assert len(blocks) >= len(C.corpus()) and any(not dd.any() for _, _, dd, _ in blocks)                 # a block without any distance symbol
    blocks += [('one symbol', eob, none, True), ('two symbols', two, none, False)]
    blocks.append(('no distance symbol', np.bincount(C.corpus()['noise'][0].ravel(), minlength=286) + eob, none, True))
    for seed in CL_DEEP_SEEDS:
        ll = _split_counts(seed)
        assert P.code_lengths(_cl_counts(P.code_lengths(ll, 15), none), 40).max() > 7, seed            # the case keeps covering the limiter
        blocks.append((f'deep code-length code {seed}', ll, none, True))
    deep = sum(P.code_lengths(_cl_counts(P.code_lengths(ll, 15), P.code_lengths(dd, 15)), 40).max() > 7 for _, ll, dd, _ in blocks)
    assert deep >= len(CL_DEEP_SEEDS)                                                                     # (ramp_avg's block is one more)
    vectors = [(7, fib[:19]), (15, fib[:30]), (7, [0, 4, 0]), (15, [0, 4, 0]), (7, [3, 0, 4]), (15, [3, 0, 4]), (15, [0] * 30)]
    assert P.code_lengths(fib[:19], 40).max() == 18 and P.code_lengths(fib[:30], 40).max() == 29
    rng = np.random.default_rng(11)
    limited = {7: 0, 15: 0}
    for kind in ('uniform', 'sparse', 'fibonacci', 'geometric'):
        for n, limit in ((19, 7), (30, 7), (19, 15), (30, 15), (286, 15)):
            for _ in range(20):
                counts = [int(v) for v in _random_counts(rng, kind, n)]
                vectors.append((limit, counts))
                limited[limit] += int(P.code_lengths(counts, 40).max() > limit)
    assert len(vectors) >= 400 and limited[7] > 0 and limited[15] > 0, limited
    records = tmp_path / 'records.txt'
    with open(records, 'w') as f:
        for _, ll, dd, final in blocks:
            f.write('H %d %s %s\n' % (final, ' '.join(map(str, ll.tolist())), ' '.join(map(str, dd.tolist()))))
        for limit, counts in vectors:
            f.write('L %d %d %s\n' % (limit, len(counts), ' '.join(map(str, counts))))
        f.write('S\n')
    run = subprocess.run([exe, str(records)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == '', run.stderr[-2000:]
    lines = [ln.split() for ln in run.stdout.splitlines()]
    assert len(lines) == 7 * len(blocks) + len(vectors) + 7
    ints = lambda ln, tag: [int(v) for v in ln[1:]] if ln[0] == tag else pytest.fail(f'{ln[0]} where {tag} was expected')   # noqa: E731
    for k, (name, ll, dd, final) in enumerate(blocks):
        got = lines[7 * k:7 * k + 7]
        ll_len, d_len = P.code_lengths(ll, 15), P.code_lengths(dd, 15)
        assert ints(got[0], 'll') == ll_len.tolist() and ints(got[1], 'dd') == d_len.tolist(), name
        assert ints(got[2], 'llcode') == P.canonical(ll_len).tolist() and ints(got[3], 'dcode') == P.canonical(d_len).tolist(), name
        hdr, (hlit, hdist, hclen, cl_len) = P.dynamic_header(ll_len, d_len, final)
        assert got[4][0] == 'hdr' and int(got[4][1]) == sum(n for _, n in hdr), name
        assert got[4][2] == P._pack([v for v, _ in hdr], [n for _, n in hdr]).hex(), name
        assert ints(got[5], 'h') == [hlit, hdist, hclen] and ints(got[6], 'cl') == cl_len.tolist(), name
    for (limit, counts), ln in zip(vectors, lines[7 * len(blocks):]):
        assert ints(ln, 'len') == P.code_lengths(counts, limit).tolist(), (limit, counts)
    sym = dict((ln[0], [int(v) for v in ln[1:]]) for ln in lines[-7:])
    assert sym['lensym'] == [v for n in range(3, 259) for v in (257 + int(P._LEN_SYM[n]), int(P._LEN_EB[n]), int(P._LEN_EX[n]))]
    assert sym['distsym'] == [v for d in range(1, 32769) for v in P.dist_code(d)]
    assert sym['take'] == [P.take(n) for n in range(601)]
    d_ext = dict(P.dist_code(d)[:2] for d in range(1, 32769))
    assert sym['llextra'] == [0] * 257 + P.LEXT and sym['dextra'] == [d_ext[s] for s in range(30)]
    fixed = P.canonical(list(P.FIXED_LL) + [8, 8])[:286]
    assert sym['fixed'] == [int(v) for s in range(286) for v in (fixed[s], P.FIXED_LL[s])] and sym['rev0'] == [0]


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------
def test_sizes_against_the_fixed_form_and_pil():
    ratios = {}
    for name in C.PHOTO + C.SMOOTH:
        e = C.encoded(name)
        raw, B = P.raw_rows(*C.corpus()[name])
        fixed = png_ref.encode(raw)[0]                                           # today's form on the same bytes: filter 0, one fixed block
        assert len(e['stream']) < len(fixed), name
        ratios[name] = len(_file(name)) / _pil_bytes(_pixels(name))
        print(name, 'model', len(_file(name)), 'fixed form', len(fixed), 'ratio to PIL', round(ratios[name], 3))
    assert max(ratios[k] for k in C.PHOTO) <= PHOTO_WORST + 0.05
    assert max(ratios[k] for k in C.SMOOTH) <= SMOOTH_WORST + 0.05
    assert len(C.encoded('bike_rgba')['stream']) * 2 < len(png_ref.encode(P.raw_rows(*C.corpus()['bike_rgba'])[0])[0])   # a photograph: less than half


# ---- the reference's recorded bytes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', GOLDEN, ids=os.path.basename)
def test_rgba_cases_of_the_reference(path):
    z = np.load(path)
    frame, planes = z['frame'], z['planes'].astype(np.float32)
    n = 0
    for key in z.files:
        if not key.startswith('rgba_'):
            continue
        targets = [] if key == 'rgba_none' else [int(v) for v in key.split('_')[1:]]
        _, a = M.composite('alpha', planes=planes, targets=targets)
        e = P.encode(frame, a)
        im = Image.open(io.BytesIO(PNG.assemble_image(e['stream'], frame.shape[0], frame.shape[1], 4)))
        assert im.mode == 'RGBA' and np.array_equal(np.array(im), z[key]), key
        n += 1
    assert n >= 1 or 'rgba' not in ''.join(z.files)


# ---- descriptor and arguments ----------------------------------------------------------------------------------------------------------
@pytest.fixture
def executor():
    from mock_exec_png_photo import PngPhotoMockExecutor
    ex = PngPhotoMockExecutor()
    ex.per_sample_conv = True
    _lib.set_executor_for_testing(M.MatteExecutor(ex))
    yield ex
    _lib.set_executor_for_testing(None)


def test_descriptor_and_argument_checks(executor):
    H, W = 5, 9
    room = torch.zeros((H, 3 * W + 5), dtype=torch.uint8)
    frame = room[:, :3 * W].view(H, W, 3)
    plane = torch.arange(H * W, dtype=torch.uint8).view(H, W)
    cap, words = O.OpList.png_photo_capacity(H, W, 4), O.OpList.png_photo_scratch_words(H, W, 4)
    stream, status, scratch = torch.zeros(cap, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32), torch.zeros(words, dtype=torch.int32)
    ol = O.OpList()
    ol.png_photo(frame, stream, status, scratch, last=plane)
    ol.png_photo(plane, stream, status, scratch)
    ol.run()
    assert executor.png_photo_calls[0][:3] == (H, W, 4) and executor.png_photo_calls[1][:3] == (H, W, 1)
    want = P.encode(plane.numpy())
    assert status.tolist()[0] == want['size'] and bytes(stream[:want['size']].numpy()) == want['stream']
    assert O.OpList.PNG_PHOTO_ROW_LIMIT == P.ROW_LIMIT and O.OpList.PNG_PHOTO_BAND == P.R
    assert O.OpList.png_photo_fits(4095, 4) and not O.OpList.png_photo_fits(4096, 4) and O.OpList.png_photo_fits(16383, 1)
    for bad in (dict(src=plane.float()), dict(src=plane[:, ::2]), dict(src=torch.zeros((H, W, 4), dtype=torch.uint8)), dict(last=plane[:, :4]),
                dict(last=plane.int()), dict(stream=stream[1:]), dict(status=status[:3]), dict(scratch=scratch[:words - 8]),
                dict(src=torch.zeros((2, 16384), dtype=torch.uint8)), dict(ldrow=3 * W - 1), dict(stream=stream.int())):
        kw = dict(src=frame, stream=stream, status=status, scratch=scratch, last=plane)
        kw.update(bad)
        with pytest.raises(ValueError):
            O.OpList().png_photo(kw.pop('src'), kw.pop('stream'), kw.pop('status'), kw.pop('scratch'), **kw)
    src = open(os.path.join(HERE, '..', 'include', 'cutie_hip.h')).read()
    assert 'flags == 16384' in src and 'bit 8 (value 256)' in src and f'CUTIE_PNG_PHOTO_ROW_LIMIT {P.ROW_LIMIT}' in src
    kern = open(os.path.join(HERE, '..', 'cutie_amd', 'csrc', 'png_photo.hip')).read()
    assert f'#define PPH_MINMATCH {P.MINMATCH} ' in kern and f'#define PPH_R {P.R} ' in kern and f'#define PPH_RUNCAP {P.RUNCAP} ' in kern


def test_a_stale_library_is_named(monkeypatch):
    monkeypatch.setattr(_lib, '_executor', None)
    monkeypatch.setattr(_lib, 'has_png_photo', lambda: False)
    with pytest.raises(_lib.HipLibraryError, match='16384'):
        O.OpList().png_photo(torch.zeros((2, 2), dtype=torch.uint8), None, None, None)


def test_assemble_keeps_its_bytes_and_the_new_container():
    ids = C.corpus()['blocks'][0]
    stream = png_ref.encode(ids)[0]
    assert PNG.assemble(stream, *ids.shape, None) == PNG.assemble_image(stream, *ids.shape, 1)      # colour type 0: the same file
    assert PNG.COLOR_TYPES == P.COLOR_TYPE
    for bad in (0, 5):
        with pytest.raises(ValueError):
            PNG.assemble_image(stream, 2, 2, bad)
    with pytest.raises(ValueError):
        PNG.assemble_image(stream, 0, 2, 1)


# ---- saver and parser -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('egress', ['host', 'device'])
def test_saver_writes_cutouts_and_dynamic_planes(tmp_path, executor, egress):
    import png_photo_saver_case as S
    S.run_and_check(str(tmp_path), 'cpu', egress)
    per_frame = [(S.H, S.W, 1)] * 3 + [(S.H, S.W, 4)]                            # two soft masks, the matte, the cut-out
    dyn_calls = executor.png_photo_calls[:12]
    assert [c[:3] for c in dyn_calls] == per_frame * 3 and all(c[3][2] == 0 for c in dyn_calls)
    assert len(executor.png_photo_calls) == 12                                   # the run with the fixed codes issued none


class _Recorder:
    """Wraps an executor and keeps (kind, flags) of every descriptor."""
    is_mock = True

    def __init__(self, inner):
        self.inner, self.ops = inner, []

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def stream(self):
        return 0

    def run(self, arr):
        for rec in arr:
            self.ops.append((int(rec['kind']), int(rec['flags'])))
        return self.inner.run(arr)


def test_default_saver_records_what_it_did(tmp_path, executor):
    """Without the new arguments: the same descriptors as before -- the planes go through the id planes' encoder (flags 8)."""
    import png_photo_saver_case as S
    rec = _Recorder(_lib.get_executor())
    _lib.set_executor_for_testing(rec)
    S.run(str(tmp_path / 'a'), 'cpu', egress='device', alpha_matte=True, soft_masks=True)
    per_frame = [(36, 4 | 8), (36, 256), (36, 512), (36, 8), (36, 8), (36, 8)]
    assert rec.ops == per_frame * 3
    rec.ops.clear()
    S.run(str(tmp_path / 'b'), 'cpu', egress='device', alpha_matte=True, soft_masks=True, cutout=True, png_codes='dynamic')
    assert rec.ops == ([(36, 4 | 8), (36, 256), (36, 512)] + [(36, 16384)] * 4) * 3
    rec.ops.clear()
    S.run(str(tmp_path / 'c'), 'cpu', egress='device', cutout=True)               # the cut-out alone: the matte launch and one encode
    assert rec.ops == [(36, 4 | 8), (36, 256), (36, 16384)] * 3
    assert sorted(os.listdir(tmp_path / 'c' / 'vid')) == ['00000.png', '00001.png', '00002.png', 'cutout']


def test_a_frame_beyond_the_row_limit_goes_through_pil(tmp_path, executor, monkeypatch, caplog):
    import logging
    import png_photo_saver_case as S
    monkeypatch.setattr(O.OpList, 'PNG_PHOTO_ROW_LIMIT', 4 * S.W)                # RGBA rows no longer fit; grey rows do
    with caplog.at_level(logging.WARNING):
        files = S.run(str(tmp_path / 'wide'), 'cpu', cutout=True, alpha_matte=True, png_codes='dynamic')
    warned = [r for r in caplog.records if 'cut-outs' in r.getMessage()]
    assert len(warned) == 1                                                      # logged once
    assert all(c[2] == 1 for c in executor.png_photo_calls)                      # only the matte went through the stage
    for t, fr in enumerate(S.frames()):
        cut = np.array(Image.open(files[f'vid/cutout/{t:05d}.png']))
        assert cut.shape == (S.H, S.W, 4) and np.array_equal(cut[..., :3], fr)
        assert np.array_equal(cut[..., 3], np.array(Image.open(files[f'vid/alpha/{t:05d}.png'])))


def test_bad_arguments_are_refused(tmp_path, executor):
    import png_photo_saver_case as S
    with pytest.raises(ValueError, match='png_codes'):
        S.saver(str(tmp_path), 'cpu', png_codes='optimal')
    from cutie_amd.inference.object_manager import ObjectManager
    om = ObjectManager()
    om.add_new_objects([1])
    with pytest.raises(ValueError, match='use_long_id'):
        RU.ResultSaver(str(tmp_path), 'v', dataset='generic', object_manager=om, use_long_id=True, cutout=True, processor=object())
    with pytest.raises(ValueError, match='processor'):
        RU.ResultSaver(str(tmp_path), 'v', dataset='generic', object_manager=om, use_long_id=False, cutout=True)
    s = S.saver(str(tmp_path), 'cpu', cutout=True)
    try:
        with pytest.raises(ValueError, match='process_merged'):
            s.process_merged([S.planes(0)], '00000.jpg', (S.H, S.W))
        with pytest.raises(ValueError, match='path_to_image or image_u8'):          # the cut-out needs the frame
            s.process(S.planes(0), '00000.jpg', resize_needed=True, shape=(S.H, S.W))
    finally:
        s.end()
    s = S.saver(str(tmp_path), 'cpu')                                            # the defaults: nothing new is on
    try:
        assert not s.cutout and s.png_codes == 'fixed' and RU.PNG_CODES == ('fixed', 'dynamic')
    finally:
        s.end()


def test_process_video_parser(capsys):
    from cutie_amd.process_video import arg_parser
    base = ['-v', 'v', '-m', 'm', '-o', 'o']
    a = arg_parser().parse_args(base)
    assert not a.cutout and a.png_codes == 'fixed'
    a = arg_parser().parse_args(base + ['--cutout', '--png-codes', 'dynamic', '--target-objects', '2'])
    assert a.cutout and a.png_codes == 'dynamic' and a.target_objects == [2]
    for bad in (['--png-codes', 'best'], ['--png-codes'], ['--vis', 'rgba']):
        with pytest.raises(SystemExit):
            arg_parser().parse_args(base + bad)
    capsys.readouterr()
