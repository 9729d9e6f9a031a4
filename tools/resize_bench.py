"""The PIL-exact bilinear resize (wd_resize_bilinear_u8) on a 1920x1280 frame, and the image loader with --resize on both routes.

    python tools/resize_bench.py [--frames 200] [--rounds 3] > profiles/resize.txt

Part 1, one frame, device events around the C entry point: both passes, each pass alone, against PIL's Image.resize on one thread, against
the bytes the passes move (in + 2 x intermediate + out) at 8 TB/s, and against ops.jpeg_decode / ops.autocontrast_ of the same frame.
Part 2, ImageLoader over JPEG frames with resize=800, auto_contrast=True, 4 workers and no detector: frames/s of resize_on='host' (PIL
on the loader threads) and resize_on='gpu', alternating after a warm-up of both, and the bytes each route sends over PCIe per frame."""
import argparse
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from waymo_2d_tracking_amd.detnet.inference import ImageLoader, resize_size          # noqa: E402
from waymo_2d_tracking_amd.detnet.nn import ops                                      # noqa: E402

H, W = 1280, 1920
HBM_BYTES_PER_S = 8e12


def frame(seed):
    """photo-like: low-frequency structure + sensor noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = 128 + 90 * np.sin(xx[..., None] / (40.0 + seed) + np.arange(3)) * np.cos(yy[..., None] / 55.0) + rng.normal(0, 6, (H, W, 3))
    return np.clip(img, 8, 240).astype(np.uint8)


def device_us(fn, reps=50, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def entry_point(src, oh, ow):
    """A closure that calls wd_resize_bilinear_u8 with everything prepared (output, workspace, tables, ctypes arguments): what the
    events see is the launches, not torch's allocator or the Python front-end."""
    import ctypes as C
    from waymo_2d_tracking_amd import _lib
    lib = _lib.lib()
    h, w = src.shape[:2]
    xb, xc = ops.resize_tables(w, ow, src.device) if w != ow else (None, None)
    yb, yc = ops.resize_tables(h, oh, src.device) if h != oh else (None, None)
    need = lib.wd_resize_bilinear_u8_workspace(C.c_int(h), C.c_int(w), C.c_int(oh), C.c_int(ow))
    keep = (torch.empty((oh, ow, 3), dtype=torch.uint8, device=src.device), torch.empty(max(need, 1), dtype=torch.uint8, device=src.device))
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                # noqa: E731
    args = (p(src), C.c_int(h), C.c_int(w), p(keep[0]), C.c_int(oh), C.c_int(ow), p(xb), p(xc), p(yb), p(yc), p(keep[1]), C.c_size_t(need),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))

    def call(keep=keep):
        _lib.check(lib.wd_resize_bilinear_u8(*args), 'wd_resize_bilinear_u8')
    return call


def one_frame(img, jpeg):
    from PIL import Image
    dev = torch.from_numpy(img).cuda()
    pil = Image.fromarray(img)
    for name, (oh, ow) in (('--resize 800', resize_size(W, H, 800)), ('x0.5', (H // 2, W // 2))):
        both = device_us(entry_point(dev, oh, ow))
        hor = device_us(entry_point(dev, H, ow))
        mid = ops.resize_bilinear_u8(dev, H, ow)
        ver = device_us(entry_point(mid, oh, ow))
        assert np.array_equal(ops.resize_bilinear_u8(dev, oh, ow).cpu().numpy(), np.asarray(pil.resize((ow, oh), Image.BILINEAR)))
        t0 = time.perf_counter()
        for _ in range(5):
            pil.resize((ow, oh), Image.BILINEAR)
        pil_ms = (time.perf_counter() - t0) / 5 * 1e3
        moved = H * W * 3 + 2 * H * ow * 3 + oh * ow * 3
        floor_us = moved / HBM_BYTES_PER_S * 1e6
        print('%dx%d -> %dx%d (%s): both passes %.1f us, horizontal alone '
              '%.1f us, vertical alone %.1f us; PIL on one thread %.1f ms = %.0fx; %.2f MB moved = %.1f us at 8 TB/s, the two passes take '
              '%.1fx that' % (W, H, ow, oh, name, both, hor, ver, pil_ms, pil_ms * 1e3 / both, moved / 1e6, floor_us, both / floor_us))
    dec = device_us(lambda: ops.jpeg_decode(jpeg), reps=20, warmup=3)
    con = device_us(lambda: ops.autocontrast_(dev), reps=50)
    oh, ow = resize_size(W, H, 800)
    res = device_us(entry_point(dev, oh, ow))
    print('the same frame (%d JPEG bytes): ops.jpeg_decode %.1f us per call (it synchronises), ops.autocontrast_ %.1f us, resize to %dx%d %.1f us'
          ' -> resizing a frame costs %s than decoding it' % (len(jpeg), dec, con, ow, oh, res, 'less' if res < dec else 'MORE'))


def loader_fps(items, route):
    t0 = time.perf_counter()
    n = 0
    for _, t, _ in ImageLoader(items, 800, None, workers=4, auto_contrast=True, decoder='gpu', resize_on=route):
        n += 1
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--files', type=int, default=8, help='distinct JPEG files the frames cycle through')
    args = ap.parse_args()
    from PIL import Image
    print('device:', torch.cuda.get_device_name(0), '| PIL', Image.__version__, '| torch', torch.__version__)
    imgs = [frame(s) for s in range(args.files)]
    blobs = []
    for img in imgs:
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, 'JPEG', quality=90, subsampling=2)
        blobs.append(buf.getvalue())
    one_frame(imgs[0], blobs[0])
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i, b in enumerate(blobs):
            paths.append(os.path.join(d, '%d.jpg' % i))
            with open(paths[-1], 'wb') as f:
                f.write(b)
        items = [(i, paths[i % len(paths)]) for i in range(args.frames)]
        a = [t.cpu() for _, t, _ in ImageLoader(items[:len(paths)], 800, None, auto_contrast=True)]
        b = [t.cpu() for _, t, _ in ImageLoader(items[:len(paths)], 800, None, auto_contrast=True, resize_on='gpu')]
        assert all(torch.equal(x, y) for x, y in zip(a, b)), 'the two routes differ'
        for route in ('host', 'gpu'):
            loader_fps(items[:32], route)                                      # warm-up of both routes
        rates = {'host': [], 'gpu': []}
        for _ in range(args.rounds):
            for route in ('host', 'gpu'):
                rates[route].append(loader_fps(items, route))
    oh, ow = resize_size(W, H, 800)
    jpeg_bytes = sum(len(b) for b in blobs) / len(blobs)
    print('ImageLoader, %d JPEG frames 1920x1280 (quality 90, 4:2:0), resize=800, auto_contrast=True, 4 workers, no detector, frames equal on both routes:'
          % args.frames)
    for route in ('host', 'gpu'):
        print("  resize_on='%s': %s frames/s (rounds alternate host, gpu)" % (route, ' / '.join('%.0f' % r for r in rates[route])))
    print('  PCIe per frame: host route %.2f MB (the resized %dx%d frame), device route %.2f MB (the file bytes)' % (oh * ow * 3 / 1e6, ow, oh, jpeg_bytes / 1e6))
    hm, gm = sorted(rates['host'])[len(rates['host']) // 2], sorted(rates['gpu'])[len(rates['gpu']) // 2]
    print('  median %.0f vs %.0f frames/s -> the device route %s the host route (%.2fx)' % (gm, hm, 'out-feeds' if gm > hm else 'does NOT out-feed', gm / hm))


if __name__ == '__main__':
    main()
