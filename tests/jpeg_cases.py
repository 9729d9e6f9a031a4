"""Synthetic JPEG files for the decoder tests (encoded with PIL, i.e. by the libjpeg-turbo whose decoder is the reference)."""
import io

import numpy as np


def synth(h, w, kind, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 0:                                                     # smooth ramps
        img = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 3) % 256], -1)
    elif kind == 1:                                                   # white noise: long codes, every coefficient alive
        img = rng.integers(0, 256, (h, w, 3))
    else:                                                             # photo-like: low-frequency structure + sensor noise
        img = (128 + 100 * np.sin(xx[..., None] / 5.0 + np.arange(3)) * np.cos(yy[..., None] / 7.0)).clip(0, 255)
        img = img + rng.normal(0, 12, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(arr, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, 'JPEG', **kw)
    return buf.getvalue()


def pil_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))


def small_cases():
    """(name, file bytes): sizes around the MCU edges x subsampling x quality x restart interval x optimised tables."""
    out = []
    sizes = [(16, 16), (8, 8), (1, 1), (2, 3), (17, 33), (48, 64), (50, 70), (5, 100), (100, 5), (31, 47), (64, 3), (3, 64), (9, 6)]
    for i, (h, w) in enumerate(sizes):
        for sub in (0, 1, 2):
            kind, q, ri = (i + sub) % 3, (30, 75, 95, 100)[(i + sub) % 4], (0, 1, 3)[(i + 2 * sub) % 3]
            kw = dict(quality=q, subsampling=sub)
            if ri:
                kw['restart_marker_blocks'] = ri
            out.append(('%dx%d_s%d_q%d_r%d_k%d' % (h, w, sub, q, ri, kind), encode(synth(h, w, kind, seed=i), **kw)))
    for h, w in ((16, 16), (17, 33), (5, 7)):
        out.append(('gray_%dx%d' % (h, w), encode(synth(h, w, 2, seed=5)[..., 0], quality=80)))
    out.append(('optimised_40x56', encode(synth(40, 56, 2, seed=9), quality=85, optimize=True)))
    out.append(('optimised_noise_33x20', encode(synth(33, 20, 1, seed=9), quality=100, subsampling=0, optimize=True)))
    return out


def medium_cases():
    """larger files (thousands of subsequences, several workgroups of the synchronisation kernel)"""
    out = []
    for (h, w, sub, q, ri, kind) in [(240, 320, 2, 90, 0, 2), (241, 323, 2, 75, 0, 2), (200, 300, 0, 100, 0, 1), (300, 200, 1, 95, 0, 1),
                                     (256, 384, 2, 85, 5, 2), (886, 1920, 2, 90, 0, 2), (480, 640, 2, 100, 0, 1)]:
        kw = dict(quality=q, subsampling=sub)
        if ri:
            kw['restart_marker_blocks'] = ri
        out.append(('%dx%d_s%d_q%d_r%d_k%d' % (h, w, sub, q, ri, kind), encode(synth(h, w, kind, seed=h), **kw)))
    return out


def tiled(h, w, channels, seed=0):
    """periodic content: one random 8x8 gray block (channels 1) or one random 16x16 RGB block (channels 3) repeated over the image.
    Every MCU then codes the same bits, so a decoder that starts out of step stays out of step by the same amount for ever: such a
    stream does not self-synchronise, and the truth only moves through it from the segment start, one workgroup per launch."""
    rng = np.random.default_rng(seed)
    tile = rng.integers(0, 256, (8, 8))
    if channels == 1:
        return np.tile(tile, (-(-h // 8), -(-w // 8)))[:h, :w].astype(np.uint8)
    tile = rng.integers(0, 256, (16, 16, 3))                          # drawn behind the gray tile, from the same generator
    return np.tile(tile, (-(-h // 16), -(-w // 16), 1))[:h, :w].astype(np.uint8)


def encode_optimised(arr, **kw):
    """encode(optimize=True) for files larger than PIL's output block ("Suspension not allowed here" otherwise)"""
    from PIL import ImageFile
    keep = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(keep, 4 * arr.size + (1 << 16))
    try:
        return encode(arr, optimize=True, **kw)
    finally:
        ImageFile.MAXBLOCK = keep


def _cached(fn):
    """the case families are searched / encoded once per process; callers get a fresh list of the same (name, bytes) pairs"""
    memo = []

    def wrapper():
        if not memo:
            memo.append(fn())
        return list(memo[0])
    wrapper.__doc__ = fn.__doc__
    wrapper.__name__ = fn.__name__
    return wrapper


# ---- marker-level view of a file: plain Python, independent of csrc/jpeg_host.h ---------------------------------------------------
SUB_BYTES = 128                                                       # one subsequence of the GPU decoder (jpeg_core.h SUB_BITS / 8)
GROUP = 256                                                           # subsequences per workgroup of the synchronisation kernel


def segment_byte_counts(data):
    """unstuffed bytes of entropy-coded data per restart segment (FF 00 counts one byte, fill FFs none; RSTn ends a segment, any
    other marker the scan)"""
    data = bytes(data)
    assert data[:2] == b'\xff\xd8'
    pos = 2
    while True:                                                       # marker segments up to and including SOS
        while data[pos] != 0xFF:
            pos += 1
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        if 0xD0 <= m <= 0xD7 or m == 0x01:
            continue
        assert m != 0xD9, 'no scan'
        n = (data[pos] << 8) | data[pos + 1]
        pos += n
        if m == 0xDA:
            break
    counts, cur = [], 0
    while True:
        q = data.find(b'\xff', pos)
        if q < 0 or q + 1 >= len(data):
            cur += (len(data) if q < 0 else q) - pos
            break
        cur += q - pos
        nb = data[q + 1]
        if nb == 0:
            cur += 1
            pos = q + 2
        elif nb == 0xFF:
            pos = q + 1
        elif 0xD0 <= nb <= 0xD7:
            counts.append(cur)
            cur = 0
            pos = q + 2
        else:
            break
    counts.append(cur)
    return counts


def subsequence_layout(data):
    """(first_sub, nsub): first_sub[s] = first subsequence of restart segment s (every segment starts on a subsequence boundary),
    first_sub[-1] = nsub"""
    first = [0]
    for b in segment_byte_counts(data):
        first.append(first[-1] + -(-b // SUB_BYTES))
    return first, first[-1]


def round_bound(nsub, group=GROUP):
    """launches of the synchronisation kernel a stream of nsub subsequences can need at most: a workgroup reads its predecessor's
    exit state at entry, so the truth crosses at least one workgroup per launch (launch 1 settles workgroup 0; launch g + 1 settles
    workgroup g), and the host looks at the chain after launches 2, 6, 10, ..."""
    groups = -(-nsub // group)
    return 2 + 4 * max(0, -(-(groups - 2) // 4))


def emulator(tmpdir):
    """builds tests/native/jpeg_sync_emul.cpp (the decoder's entropy stage thread by thread on the CPU) with g++ into tmpdir;
    returns run(data, group=256) -> (coefficients (blocks, 64) int16 in scan order, rounds, geometry[10])"""
    import ctypes
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(str(tmpdir), 'libjpeg_emul.so')
    subprocess.run(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-o', so, os.path.join(root, 'tests', 'native', 'jpeg_sync_emul.cpp')],
                   check=True)
    lib = ctypes.CDLL(so)

    def run(data, group=256):
        cap = 1 << 17
        coef = np.zeros((cap, 64), np.int16)
        rounds, total = ctypes.c_int(0), ctypes.c_int(0)
        geo = (ctypes.c_int * 10)()
        err = ctypes.create_string_buffer(256)
        rc = lib.jpeg_emul_coefficients(data, ctypes.c_long(len(data)), group, coef.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(cap),
                                        ctypes.byref(rounds), ctypes.byref(total), geo, err, 256)
        if rc:
            raise RuntimeError(err.value.decode())
        return coef[:total.value], rounds.value, list(geo)
    return run


def sequential_coefficients(data):
    """coefficients of the sequential restatement (oracle/jpeg_ref.py) in the emulator's layout: (blocks in scan order, 64) int16"""
    from oracle import jpeg_ref as J
    info = J.parse(data)
    planes = J.decode_coefficients(info)
    hmax, vmax, shape, mx, my = J.geometry(info)
    out = []
    for ci, (h, v) in enumerate(shape):                               # [mcu, block in MCU of this component, 64]
        p = planes[ci].reshape(my, v, mx, h, 64).transpose(0, 2, 1, 3, 4).reshape(my * mx, v * h, 64)
        out.append(p)
    return np.concatenate(out, axis=1).reshape(-1, 64)


# ---- streams that need more than the two fixed synchronisation launches ------------------------------------------------------------
SLOW_SYNC = [                                                         # (channels, h, w, quality, subsampling, restart_marker_blocks)
    (1, 256, 256, 100, None, 0),
    (1, 384, 384, 100, None, 0),
    (1, 640, 640, 75, None, 0),
    (3, 256, 256, 100, 0, 0),
    (3, 384, 384, 100, 2, 0),
    (3, 250, 390, 100, 1, 0),                                         # not whole MCUs
    (3, 384, 384, 100, 2, 400),
]


def _slow_name(ch, h, w, q, sub, ri, opt=False):
    return 'tiled_%s_%dx%d_q%d%s%s%s' % ('gray' if ch == 1 else 'rgb', h, w, q, '' if sub is None else '_s%d' % sub,
                                         '_r%d' % ri if ri else '', '_opt' if opt else '')


def _slow_file(ch, h, w, q, sub, ri, opt=False):
    kw = dict(quality=q)
    if sub is not None:
        kw['subsampling'] = sub
    if ri:
        kw['restart_marker_blocks'] = ri
    arr = tiled(h, w, ch)
    return encode_optimised(arr, **kw) if opt else encode(arr, **kw)


# optimize=True candidates (<= 400 x 400); the first whose stream spans 7 to 9 workgroups is taken.  tests/test_jpeg_cases.py pins
# its emulated rounds.
SLOW_SYNC_OPTIMISED = [(3, 400, 400, 100, 2, 0), (3, 384, 384, 100, 2, 0), (3, 320, 320, 100, 0, 0), (3, 288, 288, 100, 0, 0)]


@_cached
def slow_sync_cases():
    """(name, file bytes): periodic content at seven sizes / samplings / restart intervals - 7 to 9 workgroups of the
    synchronisation kernel and 10 emulated rounds each, but for the smallest (4 workgroups, 6 rounds) - and one with optimised
    Huffman tables when this encoder gives one of 7 to 9 workgroups"""
    out = [(_slow_name(*c), _slow_file(*c)) for c in SLOW_SYNC]
    for c in SLOW_SYNC_OPTIMISED:
        data = _slow_file(*c, opt=True)
        if 7 <= -(-subsequence_layout(data)[1] // GROUP) <= 9:
            out.append((_slow_name(*c, opt=True), data))
            break
    return out


# ---- restart segments that end on, one byte past, or one byte before a subsequence boundary ----------------------------------------
EDGE_RESIDUES = (0, 1, 127)
EDGE_POSITIONS = ('only', 'middle', 'last')


def segment_edge_classes(data):
    """{(residue, position)}: which of the nine classes the segments of a file fall into.  'only' = a file of one segment,
    'last' = the last of several, 'middle' = neither the first nor the last of several."""
    counts = segment_byte_counts(data)
    out = set()
    for s, b in enumerate(counts):
        if b % SUB_BYTES not in EDGE_RESIDUES:
            continue
        if len(counts) == 1:
            out.add((b % SUB_BYTES, 'only'))
        elif s == len(counts) - 1:
            out.add((b % SUB_BYTES, 'last'))
        elif s > 0:
            out.add((b % SUB_BYTES, 'middle'))
    return out


def _edge_candidates():
    """the deterministic stream of small files the search walks: 24..84 x 24..114, noise or photo-like, three qualities, three
    subsamplings, with and without a restart interval of 2 MCUs"""
    n = 0
    while True:
        rng = np.random.default_rng(1000 + n)
        h, w = int(rng.integers(24, 85)), int(rng.integers(24, 115))
        kind, q, sub, ri = (1, 2)[n % 2], (60, 85, 95)[(n // 2) % 3], (n // 6) % 3, (0, 2)[(n // 18) % 2]
        kw = dict(quality=q, subsampling=sub)
        if ri:
            kw['restart_marker_blocks'] = ri
        yield '%dx%d_s%d_q%d_r%d_k%d_n%d' % (h, w, sub, q, ri, kind, n), h * w, encode(synth(h, w, kind, seed=n), **kw)
        n += 1


EDGE_SEARCH_LIMIT = 6000


@_cached
def segment_edge_cases():
    """(name, file bytes), nine files: for every residue of the segment length mod 128 in {0 (no padding at all), 1 (a subsequence
    of 8 real bits), 127 (8 bits of padding)} one file whose only segment, one whose middle segment and one whose last segment has
    it.  Names start with 'seg<residue>_<position>_'.  The first hit of each class in the walk is taken, files of at most 5000
    pixels (the size the sequential restatement is compared with PIL at) before larger ones."""
    found = {}
    for n, (name, pixels, data) in enumerate(_edge_candidates()):
        if n >= EDGE_SEARCH_LIMIT:
            break
        for cls in segment_edge_classes(data):
            if cls not in found or (found[cls][1] > 5000 >= pixels):
                found[cls] = ('seg%d_%s_%s' % (cls[0], cls[1], name), pixels, data)
        if len(found) == 9 and all(v[1] <= 5000 for v in found.values()):
            break
    return [(found[(r, p)][0], found[(r, p)][2]) for r in EDGE_RESIDUES for p in EDGE_POSITIONS if (r, p) in found]


# ---- restart segments across the pass boundaries of the two single-workgroup scans -------------------------------------------------
RESOLVE_PASS = 8192                                                   # subsequences per pass of jpeg_resolve_kernel
SCAN_PASS = 4096                                                      # ... of jpeg_scan_kernel


def _scan_pass_file(seed, ri):
    return encode(synth(640, 648, 1, seed), quality=100, subsampling=0, restart_marker_blocks=ri)


@_cached
def scan_pass_cases():
    """(name, file bytes), three files of more than 8192 subsequences: 3 restart segments that span subsequences 4096 and 8192
    (the carried state of both scans is a live one), and 81 segments of which one starts exactly at 4096 / exactly at 8192 (the
    carry must be dropped at the first item of a pass).  The two seeds are found by search: they depend on the encoder."""
    out = [('spans_640x648_r3000_seed0', _scan_pass_file(0, 3000))]
    want = {SCAN_PASS: None, RESOLVE_PASS: None}
    for seed in range(40):
        if all(v is not None for v in want.values()):
            break
        data = _scan_pass_file(seed, 80)
        first = subsequence_layout(data)[0][:-1]
        for at in want:
            if want[at] is None and at in first:
                want[at] = ('starts_at_%d_640x648_r80_seed%d' % (at, seed), data)
    return out + [want[at] for at in (SCAN_PASS, RESOLVE_PASS) if want[at] is not None]


# ---- saturated content at very low quality: the range-limit arms of the inverse DCT -------------------------------------------------
@_cached
def low_quality_cases():
    """(name, file bytes), 12 files: a 0 / 255 checkerboard and binary noise, green channel inverted, 40x56, quality 1 / 3 / 10,
    4:4:4 and 4:2:0 - coarse quantisation of full-swing content overshoots 0..255 far in both directions"""
    h, w = 40, 56
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((yy // 3 + xx // 5) % 2) * 255).astype(np.uint8)
    noise = (np.random.default_rng(7).integers(0, 2, (h, w)) * 255).astype(np.uint8)
    out = []
    for cname, plane in (('checker', board), ('binary', noise)):
        img = np.stack([plane, 255 - plane, plane], -1)
        for q in (1, 3, 10):
            for sub in (0, 2):
                out.append(('lowq_%s_%dx%d_q%d_s%d' % (cname, h, w, q, sub), encode(img, quality=q, subsampling=sub)))
    return out


def real_world_files(limit=16):
    """JPEG files written by other encoders than PIL's - optimised Huffman tables, other quantisation tables, a restart interval of 32,
    an Adobe marker, 2x2 up to 1411x1411 - kept as fixtures under tests/golden/jpeg_other_encoders/ (sources and licences in its
    SOURCES.txt), so the tests see the same files on every machine."""
    import glob
    import os
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_other_encoders')
    return sorted(glob.glob(os.path.join(d, '*.jp*g')))[:limit]
