"""PIL-exact bilinear resize on the GPU (csrc/det_resize.hip) against the installed PIL, bit for bit, on the shapes of resize_cases.py;
memory safety with guard bytes and unaligned views; the loader's resize_on='gpu' route against the default host route."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_cases as JC                                                                      # noqa: E402
from resize_cases import CONTENTS, SHAPES, make_image, pil_resize, shape_id                  # noqa: E402

pytestmark = pytest.mark.gpu

WT_ERR_CAPACITY = 4


def _ops():
    from waymo_2d_tracking_amd.detnet.nn import ops
    return ops


def _raw_resize(src, dst, ws, ws_bytes, stream=None):
    """wd_resize_bilinear_u8 on tensors (views allowed); returns the status code."""
    from waymo_2d_tracking_amd import _lib
    ops = _ops()
    (h, w), (oh, ow) = src.shape[:2], dst.shape[:2]
    xb, xc = ops.resize_tables(w, ow, src.device) if w != ow else (None, None)
    yb, yc = ops.resize_tables(h, oh, src.device) if h != oh else (None, None)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                    # noqa: E731
    st = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return _lib.lib().wd_resize_bilinear_u8(p(src), C.c_int(h), C.c_int(w), p(dst), C.c_int(oh), C.c_int(ow), p(xb), p(xc), p(yb), p(yc),
                                            p(ws), C.c_size_t(ws_bytes), st)


@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
def test_resize_equals_pil(shape):
    ops = _ops()
    oh, ow = shape[1]
    for content in CONTENTS:
        img = make_image(shape, content)
        got = ops.resize_bilinear_u8(torch.from_numpy(img).cuda(), oh, ow).cpu().numpy()
        exp = pil_resize(img, oh, ow)
        assert got.shape == exp.shape and got.dtype == np.uint8
        assert np.array_equal(got, exp), (content, '%d of %d bytes differ' % (int((got != exp).sum()), exp.size))
        if content == 'full':
            assert int(got.min()) == 255


def test_resize_equals_pil_on_a_full_size_frame():
    ops = _ops()
    img = np.random.default_rng(5).integers(0, 256, (1280, 1920, 3), dtype=np.uint8)
    dev = torch.from_numpy(img).cuda()
    exp = torch.from_numpy(pil_resize(img, 800, 1200).copy())
    got = ops.resize_bilinear_u8(dev, 800, 1200)
    assert torch.equal(got.cpu(), exp)
    assert torch.equal(ops.resize_bilinear_u8(dev, 800, 1200).cpu(), exp)                   # a second launch repeats the answer
    assert torch.equal(dev.cpu(), torch.from_numpy(img))                                     # and the source is only read


@pytest.mark.parametrize('offset', [0, 1, 2, 3])
def test_resize_keeps_inside_its_buffers(offset):
    """Guard bytes before and after dst and after the workspace, the source a view in the middle of a larger buffer; every buffer
    starts `offset` bytes behind a 4-byte boundary, so rows and buffer ends fall on every position inside an aligned word."""
    from waymo_2d_tracking_amd import _lib
    guard = 64 + offset
    for shape in SHAPES:
        (h, w), (oh, ow) = shape
        img = make_image(shape, 'random', seed=offset)
        n_src, n_dst = h * w * 3, oh * ow * 3
        n_ws = _lib.lib().wd_resize_bilinear_u8_workspace(C.c_int(h), C.c_int(w), C.c_int(oh), C.c_int(ow))
        assert n_ws == (h * ow * 3 if (h != oh and w != ow) else 0)
        src_buf = torch.full((guard + n_src + 64,), 0xA5, dtype=torch.uint8, device='cuda')
        dst_buf = torch.full((guard + n_dst + 64,), 0x5A, dtype=torch.uint8, device='cuda')
        ws_buf = torch.full((guard + n_ws + 64,), 0x3C, dtype=torch.uint8, device='cuda')
        assert src_buf.data_ptr() % 4 == 0 and dst_buf.data_ptr() % 4 == 0 and ws_buf.data_ptr() % 4 == 0
        src = src_buf[guard:guard + n_src].view(h, w, 3)
        src.copy_(torch.from_numpy(img))
        dst = dst_buf[guard:guard + n_dst].view(oh, ow, 3)
        ws = ws_buf[guard:guard + n_ws]
        assert _raw_resize(src, dst, ws, n_ws) == 0, (shape, _lib.lib().wt_last_error())
        exp = pil_resize(img, oh, ow)
        assert np.array_equal(dst.cpu().numpy(), exp), shape
        src_all, dst_all, ws_all = src_buf.cpu().numpy(), dst_buf.cpu().numpy(), ws_buf.cpu().numpy()
        assert (dst_all[:guard] == 0x5A).all() and (dst_all[guard + n_dst:] == 0x5A).all(), shape
        assert (ws_all[:guard] == 0x3C).all() and (ws_all[guard + n_ws:] == 0x3C).all(), shape
        assert (src_all[:guard] == 0xA5).all() and (src_all[guard + n_src:] == 0xA5).all(), shape
        assert np.array_equal(src_all[guard:guard + n_src].reshape(h, w, 3), img), shape


def test_resize_on_a_side_stream():
    ops = _ops()
    shape = ((96, 130), (37, 50))
    img = make_image(shape, 'random')
    dev = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = ops.resize_bilinear_u8(dev, 37, 50)
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), pil_resize(img, 37, 50))


def test_short_workspace_is_a_capacity_error_before_any_launch():
    from waymo_2d_tracking_amd import _lib
    shape = ((61, 91), (30, 45))
    src = torch.from_numpy(make_image(shape, 'random')).cuda()
    dst = torch.full((30, 45, 3), 0x77, dtype=torch.uint8, device='cuda')
    need = 61 * 45 * 3
    ws = torch.zeros(need, dtype=torch.uint8, device='cuda')
    assert _raw_resize(src, dst, ws, need - 1) == WT_ERR_CAPACITY
    assert b'workspace_bytes' in _lib.lib().wt_last_error()
    torch.cuda.synchronize()
    assert int((dst != 0x77).sum()) == 0
    assert _raw_resize(src, dst, ws, need) == 0
    assert np.array_equal(dst.cpu().numpy(), pil_resize(src.cpu().numpy(), 30, 45))


def test_table_cache_serves_two_sizes_alternately():
    ops = _ops()
    a, b = ((48, 72), (32, 48)), ((61, 91), (30, 45))
    ia, ib = make_image(a, 'random'), make_image(b, 'random')
    da, db = torch.from_numpy(ia).cuda(), torch.from_numpy(ib).cuda()
    ea, eb = pil_resize(ia, 32, 48), pil_resize(ib, 30, 45)
    for _ in range(3):
        assert np.array_equal(ops.resize_bilinear_u8(da, 32, 48).cpu().numpy(), ea)
        assert np.array_equal(ops.resize_bilinear_u8(db, 30, 45).cpu().numpy(), eb)
    first = ops.resize_tables(72, 48, da.device)
    assert ops.resize_tables(72, 48, da.device)[0] is first[0]                              # uploaded once
    assert first[0].dtype == torch.int32 and tuple(first[0].shape) == (48, 2) and first[1].shape[1] == 5


@pytest.fixture(scope='module')
def loader_files(tmp_path_factory):
    """two 96 x 144 (width x height) JPEG files, 4:2:0 and 4:4:4, a progressive one (not decoded on the GPU -> PIL, uploaded unresized)
    and one PNG"""
    from PIL import Image
    d = tmp_path_factory.mktemp('resize_loader')
    items = []
    for i, kw in enumerate((dict(subsampling=2), dict(subsampling=0), dict(subsampling=2, progressive=True))):
        path = str(d / ('%d.jpg' % i))
        with open(path, 'wb') as f:
            f.write(JC.encode(JC.synth(144, 96, 2, seed=i) // 2 + 20, quality=85, **kw))          # a range that auto-contrast stretches
        items.append((i, path))
    png = str(d / 'x.png')
    Image.fromarray(JC.synth(144, 96, 0) // 3 + 40).save(png)
    items.append((9, png))
    return items


@pytest.mark.parametrize('resize,max_size,contrast', [(48, 60, True), (64, None, True), (48, 60, False), (64, None, False)])
def test_loader_gpu_route_equals_the_host_route(loader_files, resize, max_size, contrast):
    from waymo_2d_tracking_amd.detnet.inference import ImageLoader, resize_size
    host = list(ImageLoader(loader_files, resize, max_size, auto_contrast=contrast))
    ld = ImageLoader(loader_files, resize, max_size, auto_contrast=contrast, resize_on='gpu')
    assert ld.decoder == 'gpu' and ld.auto_contrast_in_loader == contrast
    gpu = list(ld)
    assert [g[0] for g in gpu] == [i for i, _ in loader_files]
    oh, ow = resize_size(96, 144, resize, max_size)
    assert (oh, ow) == ((60, 40) if resize == 48 else (96, 64))
    for (ia, ta, sa), (ib, tb, sb) in zip(gpu, host):
        assert ia == ib and sa == sb == (96, 144)                                            # the ORIGINAL (width, height)
        assert ta.is_cuda and ta.dtype == torch.uint8 and tuple(ta.shape) == (oh, ow, 3)
        assert torch.equal(ta.cpu(), tb.cpu()), ia
    pil = list(ImageLoader(loader_files, resize, max_size, auto_contrast=contrast, decoder='pil', resize_on='gpu'))
    for (ia, ta, sa), (ib, tb, sb) in zip(pil, host):                                        # the caller's decoder is kept; same frames
        assert sa == sb and torch.equal(ta.cpu(), tb.cpu()), ia


def test_fixed_size_resize_through_the_loader(loader_files):
    from PIL import Image
    from waymo_2d_tracking_amd.detnet import inference as I
    args = I.build_parser().parse_args(['-i', 'x', '--export', 'y.json', '--resize', '72x48', '--resize-device', 'gpu'])
    I.check_supported(args)
    size = I.parse_resize(args)
    assert size == (48, 72)
    frames = list(I.ImageLoader(loader_files, size, args.max_image_size, auto_contrast=args.auto_contrast, decoder=args.decoder,
                                resize_on=args.resize_device))
    for (image_id, t, wh), (_, path) in zip(frames, loader_files):
        exp = np.asarray(Image.open(path).convert('RGB').resize((72, 48), Image.BILINEAR))
        assert tuple(t.shape) == (48, 72, 3) and wh == (96, 144)
        assert np.array_equal(t.cpu().numpy(), exp), image_id
