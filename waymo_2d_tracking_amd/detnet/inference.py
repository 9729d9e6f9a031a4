"""Detection inference CLI - mirrors /root/reference/inference.py + /root/reference/detnet/inference.py
(flags :26-60, PredictModel :77-130, inference() :151-199), the test driver (/root/reference/detnet/trainer/test.py:189-279:
`-j N`, `--resume`, `-o`) and the JSON export (/root/reference/detnet/export.py:159-165 -> detnet/data/coco.py:229-252).

    python -m waymo_2d_tracking_amd.detnet.inference -m MODEL_FILE -i IMAGES_DIR --export submission.json \
        [--tta x1.5,hflip] [--auto-contrast=1] [-j 8] [-o OUT_DIR] [--resume OUT_DIR/detections.pkl] [--eval --annotations GT.json] \
        [--resize 800 | --resize 1200x800] [--resize-device gpu]
    python -m waymo_2d_tracking_amd.detnet.inference -m MODEL_FILE -i IMAGES_DIR --export merged.json \
        --views 'orig;x1.5,hflip' --views-method soft_nms [--views-weights 1,0.8] [--export-views VIEWS_DIR]
        (--views-method weighted_fusion_b | nmw: the merge rules of detnet.ensemble_b, float boxes)
    torchrun --nproc-per-node 8 -m waymo_2d_tracking_amd.detnet.inference ...     # the same, started by torchrun

MODEL_FILE is a `{args, kwargs, state_dict}` file of the reference or of this package (nn/__init__.py); the string
`detectron2:<yaml>` loads the detectron2 COCO checkpoint like the reference does (it must be available locally).

Multi-GPU: the reference spawns `-j N` processes with contiguous dataset shards and merges per-process shelve files
(trainer/test.py:227-270).  Here `-j N` spawns N processes (one per GPU) - or torchrun does - each takes its contiguous shard
(distributed.contiguous_split), fills a columnar prediction store (trainer/predictions.py) and rank 0 receives all rows in one
tensor gather over RCCL - no files, no collective inside the detection loop.  Image decoding (PIL, like the reference's
dataset workers) runs in a thread pool ahead of the GPU; AutoContrast runs on the GPU.
"""
import argparse
import os
import time
from pathlib import Path

import threading

import numpy as np
import torch

from .. import _lib

IMG_EXT = ('.jpg', '.jpeg', '.png', '.bmp')
FUSE_VIEW_METHODS = ('weighted_fusion_b', 'nmw')        # --views-method: the merge rules of detnet.ensemble_b (devpath.FUSE_METHODS)


def arg2bool(v):
    if isinstance(v, bool):
        return v
    return str(v).lower() in ('yes', 'true', 't', 'y', '1')


def add_test_argument(parser):
    """detnet/inference.py:26-46; flags this path cannot honour raise in check_supported()."""
    parser.add_argument('--device', default='auto', choices=['auto', 'cuda', 'cpu', 'half'])
    parser.add_argument("-m", "--model", type=str, default='detectron2:Misc/cascade_mask_rcnn_X_152_32x8d_FPN_IN5k_gn_dconv.yaml',
                        help='pre/trained model file')
    parser.add_argument("--threshold", type=float, default=0.01, help='threshold for accepting detection')
    parser.add_argument("--max-bbox", type=int, default=0, help='maximum number of bbox output per image if positive')
    parser.add_argument('--max-bbox-per-class', type=int, default=4000)
    parser.add_argument("--nms-thresh", type=float, default=0.15)
    parser.add_argument('--soft-nms', action='store_true')
    parser.add_argument('--bbox-voting', type=float, default=0)
    parser.add_argument('--tta', type=str, default='', help='Test Time Augmentation, e.g. x1.5,hflip')
    parser.add_argument("--batch-size", type=int, default=0)
    parser.add_argument("--resize", type=str)
    parser.add_argument("--max-image-size", type=int)
    parser.add_argument("--resize-device", type=str, default='host', choices=('host', 'gpu'),
                        help="(extension) where --resize runs: 'host' = PIL on the loader threads like the reference, 'gpu' = decode, auto-contrast "
                             "and resize in HIP kernels (bit-exact with PIL); 'gpu' also takes --resize WxH")
    parser.add_argument("--inflight", type=int, default=2,
                        help="(extension) detector passes in flight: each image size is captured once per lane as a hipGraph and replayed on its own "
                             "stream, results are collected one image behind; 0 = one eager call per image")
    parser.add_argument("--decoder", type=str, default='gpu', choices=('gpu', 'pil'),
                        help="JPEG decoding: 'gpu' = HIP decoder (bit-exact with PIL), 'pil' = host decode like the reference")
    parser.add_argument("--auto-contrast", type=arg2bool)
    parser.add_argument("--clahe", type=arg2bool)


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    add_test_argument(parser)
    parser.add_argument("-i", "--input", type=str, help='root directory of input images')
    parser.add_argument("-o", "--output", type=str, help='root directory of output')
    parser.add_argument("--exclusive", type=str)
    parser.add_argument('-j', '--jobs', type=int, default=1, help='number of processes = GPUs (one process per GPU)')
    parser.add_argument('--annotations', type=str, help='COCO-format ground truth for --eval')
    parser.add_argument('--resume', type=str)
    parser.add_argument('--eval', action='store_true')
    parser.add_argument('--eval-gpu', action='store_true', help='with --eval: score on the GPU (detnet/evaluate.py) instead of the host loop')
    parser.add_argument('--export', type=str, help='path of export file')
    parser.add_argument('--export-format', type=str, choices=('json',), default='json')
    parser.add_argument('--profile', action='store_true')
    parser.add_argument('--cudnn-benchmark', default=True, type=arg2bool)
    parser.add_argument('--data-root', type=str, default=None)
    parser.add_argument('--data-include-empty', action='store_true')
    parser.add_argument('--data-bgr', action='store_true')
    # several TTA views of one model, merged per (image, category) on the GPU (= --tta V --export per view + detnet.ensemble)
    parser.add_argument('--views', type=str, help="';'-separated --tta specs merged per image, e.g. 'orig;x1.2;x1.5,hflip' (needs --export)")
    parser.add_argument('--views-method', choices=('weighted_fusion', 'nms', 'soft_nms') + FUSE_VIEW_METHODS, default='weighted_fusion',
                        help='how the views are merged (detnet.ensemble -m; weighted_fusion_b and nmw: detnet.ensemble_b '
                             '-m weighted_fusion / nmw, float boxes)')
    parser.add_argument('--views-iou-thresh', type=float, default=0.5, help='IOU threshold for merging bboxes')
    parser.add_argument('--views-soft-nms-cut', type=float, default=1.0, help='cutout IoU threshold for soft nms')
    parser.add_argument('--views-min-score', type=float, default=0, help='minimal score to keep')
    parser.add_argument('--views-weights', type=str, help="per-view weights, e.g. '1,0.8' (divided by their maximum)")
    parser.add_argument('--export-views', type=str, help='directory: view<k>.json = what --tta <view k> --export writes')
    return parser


VIEW_BATCH_FRAMES = 256         # images per SlotEnsemble launch


def check_views(args):
    """--views and its flags -> (specs, --tta token lists, normalised weights), or None without --views.  Conflicting or
    unfoldable settings raise ValueError / NotImplementedError with the reason."""
    from .ensemble import normalise_weights
    from .nn.tta import foldable_view
    if not args.views:
        if args.export_views or args.views_weights:
            raise ValueError('--export-views / --views-weights need --views')
        return None
    if not args.export:
        raise ValueError('--views needs --export (the merged rows are written there)')
    for flag, on in (('--tta', args.tta), ('-o/--output', args.output), ('--resume', args.resume), ('--eval', args.eval)):
        if on:
            raise ValueError('--views cannot be combined with %s: the merged rows are wire rows (integer boxes, 5-decimal scores), '
                             'not the per-class prediction store' % flag)
    if args.jobs > 1 or int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise NotImplementedError('--views runs in one process on one GPU: -j N / torchrun are not supported with it')
    specs = [v.strip() for v in args.views.split(';')]
    views = [foldable_view(v) for v in specs]
    weights = None
    if args.views_weights:
        try:
            weights = [float(w) for w in args.views_weights.split(',')]
        except ValueError:
            raise ValueError('--views-weights: %r is not a comma-separated list of numbers' % args.views_weights)
    return specs, views, normalise_weights(weights, len(views))


def merge_view_rows(image_ids, view_rows, weights, method, iou_thresh, soft_nms_cut, min_score, batch_frames=VIEW_BATCH_FRAMES):
    """The detection rows of K views (export.detection_rows columns: image index, category, int bbox, 5-decimal score, images in
    data-set order) -> the rows `python -m detnet.ensemble view0.json ... view{K-1}.json` writes, merged on the GPU.

    Every view's rows of an image fill that image's wire slots in file order (S = the most rows any view has for one image);
    devpath.SlotEnsemble merges batch_frames images per launch.  Images come out in the ensemble CLI's order: first appearance
    over the views' kept rows, view by view (merge_inputs); inside an image categories ascend.

    method 'weighted_fusion_b' / 'nmw' gives the rows of `python -m detnet.ensemble_b ... -m weighted_fusion / nmw` between the two
    min_score filters (soft_nms_cut is ignored): the boxes stay float64 and an image's rows are ordered by descending score like
    that file's (equal 5-decimal scores: ascending category, then the group's order); the scores are numpy-rounded."""
    from ..devpath import SlotEnsemble
    F, K = len(image_ids), len(view_rows)
    fuse = method in FUSE_VIEW_METHODS
    box_dtype = np.float64 if fuse else np.int64
    empty = dict(image=np.zeros(0, np.int32), category=np.zeros(0, np.int32), bbox=np.zeros((0, 4), box_dtype), score=np.zeros(0))
    counts = [np.bincount(r['image'], minlength=F) if len(r['image']) else np.zeros(F, np.int64) for r in view_rows]
    S = int(max([1] + [int(c.max()) for c in counts if len(c)]))
    C = int(max([1] + [int(r['category'].max()) for r in view_rows if len(r['category'])]))
    if any(len(r['category']) and int(r['category'].min()) < 1 for r in view_rows):
        raise ValueError('view rows need category ids >= 1')
    pos = []
    for r, c in zip(view_rows, counts):
        img = np.asarray(r['image'], np.int64)
        if np.any(np.diff(img) < 0):
            raise ValueError('view rows must be grouped by image in data-set order')
        start = np.concatenate([[0], np.cumsum(c)[:-1]])
        pos.append(img * S + (np.arange(len(img)) - start[img]))          # slot = file order inside the image
    B = max(1, min(batch_frames, F))
    ens = SlotEnsemble(B, S, weights, C, method, iou_thresh, soft_nms_cut, min_score)
    out = ens.outputs()
    parts = []
    for b0 in range(0, F, B):
        xywhs = np.zeros((K, 5, B * S))
        cat = np.zeros((K, B * S), np.int32)
        for k, r in enumerate(view_rows):
            sel = (r['image'] >= b0) & (r['image'] < b0 + B)
            p = pos[k][sel] - b0 * S
            xywhs[k, 0:4, p] = r['bbox'][sel]
            xywhs[k, 4, p] = r['score'][sel]
            cat[k, p] = r['category'][sel]
        ens.run(torch.from_numpy(xywhs).cuda(), torch.from_numpy(cat).cuda(), out=out)
        ox, oc, on = (t.cpu().numpy() for t in out)
        n = on[:min(B, F - b0)]
        slot = np.concatenate([f * K * S + np.arange(c) for f, c in enumerate(n.tolist())]) if n.sum() else np.zeros(0, np.int64)
        parts.append(dict(image=(b0 + slot // (K * S)).astype(np.int32), category=oc[slot].astype(np.int32),
                          bbox=ox[0:4, slot].T.astype(box_dtype), score=ox[4, slot].copy()))
    rows = {k: np.concatenate([p[k] for p in parts]) if parts else empty[k] for k in empty}
    # image order of merge_inputs: first appearance over the kept rows (w > 0, h > 0, score * weight >= min_score), view by view
    seen = np.concatenate([np.asarray(r['image'], np.int64)[(r['bbox'][:, 2] > 0) & (r['bbox'][:, 3] > 0) & (r['score'] * w >= min_score)]
                           for r, w in zip(view_rows, weights)] + [np.zeros(0, np.int64)])
    present, first = np.unique(seen, return_index=True)
    rank = np.full(F, F, np.int64)
    rank[present[np.argsort(first, kind='stable')]] = np.arange(len(present))
    order = np.argsort(rank[rows['image']], kind='stable')
    if fuse:
        order = order[np.lexsort((-rows['score'][order], rank[rows['image'][order]]))]          # ensemble_b.output_rows
    return {k: v[order] for k, v in rows.items()}


def run_views(args, views_spec):
    """--views: every image is decoded once and goes through one captured detector graph lane per view (scale / flips folded into
    the pre-processing kernel); each view's rows are the rows `--tta <view> --export` writes (optionally written to
    --export-views); merge_view_rows merges them on the GPU and the native writer writes --export."""
    from . import nn as detnn
    from .export import detection_rows, write_detections_json
    from .trainer import Predictions
    specs, views, weights = views_spec
    torch.backends.cudnn.benchmark = bool(args.cudnn_benchmark)
    if args.cudnn_benchmark:
        from ..tuning import enable_gemm_tuning
        enable_gemm_tuning()
    start = time.time()
    model = detnn.load(args.model).cuda().eval()
    predicts = [PredictModel(model, dict(tta=v, max_bbox=args.max_bbox)) for v in views]
    images = list_images(args.input)
    if args.exclusive:
        images = [(i, p) for i, p in images if args.exclusive not in i]
    image_ids = [i for i, _ in images]
    index = {k: i for i, k in enumerate(image_ids)}
    stores = [Predictions(model.classnames, image_ids) for _ in views]
    sizes = np.zeros((len(image_ids), 2), np.int32)
    K = len(views)
    with torch.no_grad():
        loader = ImageLoader(images, parse_resize(args), args.max_image_size, auto_contrast=args.auto_contrast, decoder=args.decoder,
                             resize_on=args.resize_device)
        lanes = [p.stream(args.inflight) for p in predicts] if args.inflight > 0 else None
        if lanes is not None and any(l is None for l in lanes):
            lanes = None                                              # no static-shape pass: one eager call per view and image
        pending = []
        for image_id, img, (w, h) in loader:
            if args.auto_contrast and not loader.auto_contrast_in_loader:
                img = autocontrast_(img)
            sizes[index[image_id]] = (w, h)
            if lanes is None:
                for k in range(K):
                    stores[k][image_id] = predicts[k](img.unsqueeze(0))[0]
                continue
            if len(pending) >= args.inflight:
                done, tickets = pending.pop(0)
                for k in range(K):
                    stores[k][done] = lanes[k][1](tickets[k])
            pending.append((image_id, [lanes[k][0](img) for k in range(K)]))
        for done, tickets in pending:
            for k in range(K):
                stores[k][done] = lanes[k][1](tickets[k])
    image_sizes = {k: (int(sizes[i, 0]), int(sizes[i, 1])) for i, k in enumerate(image_ids)}
    view_rows = [detection_rows(st, image_sizes) for st in stores]
    if args.export_views:
        for k, r in enumerate(view_rows):
            write_detections_json(Path(args.export_views) / ('view%d.json' % k), image_ids, r)
    rows = merge_view_rows(image_ids, view_rows, weights, args.views_method, args.views_iou_thresh, args.views_soft_nms_cut,
                           args.views_min_score)
    if args.views_method in FUSE_VIEW_METHODS:
        from .ensemble_b import write_detections_json as write_float_detections_json
        write_float_detections_json(Path(args.export).with_suffix('.json'), image_ids, rows)          # float boxes, like ensemble_b
    else:
        write_detections_json(Path(args.export).with_suffix('.json'), image_ids, rows)
    print(f'inference done in {time.time() - start:.1f}s, {len(image_ids)} images, views {specs} weights {weights}, '
          f'{sum(len(r["image"]) for r in view_rows)} view rows -> {len(rows["image"])} merged rows')
    return rows


class PredictModel(torch.nn.Module):
    """detnet/inference.py:77-130: TTA wrap + optional global top-k over classes."""

    def __init__(self, model, detect_args):
        super().__init__()
        self.model = model
        if detect_args.get('tta'):
            from .nn.tta import TTA
            self.model = TTA(model, detect_args['tta'])
        self.detect_args = detect_args

    def forward(self, sample):
        return [self.post_process(d) for d in self.model.predict(sample)]

    # ---- round 6: the same results for a STREAM of images with `lanes` detector passes in flight (captured hipGraphs, nn.GraphLanePredictor) ----
    def stream(self, lanes=2):
        """A (submit, collect) pair or None when this model / TTA plan has no static-shape pass (the loop then calls forward() per image)."""
        from .nn.tta import TTA, undo_plan
        if isinstance(self.model, TTA):
            gl, plan = self.model.graph_lanes(lanes), self.model.plan
        elif hasattr(self.model, 'predict_padded') and not getattr(self.model, 'tta_min_sizes', None):
            from .nn.detectron2_det import GraphLanePredictor
            gl, plan = GraphLanePredictor(self.model, lanes=lanes), []
        else:
            gl = None
        if gl is None:
            return None

        def collect(ticket):
            det = [[b.copy() for b in gl.collect(ticket)]]
            return self.post_process(undo_plan(det, plan)[0])
        return gl.submit, collect

    def post_process(self, detections):
        max_bbox = self.detect_args.get('max_bbox', 0)
        if max_bbox > 0:
            labels = np.concatenate([[i] * len(b) for i, b in enumerate(detections)]).astype(np.int64) if detections else np.zeros(0, np.int64)
            allb = np.vstack(detections)
            if len(labels) > max_bbox:
                top = np.argsort(-allb[:, 0], kind='stable')[:max_bbox]
                allb, labels = allb[top], labels[top]
                detections = [allb[labels == i] for i in range(len(detections))]
        return detections


def load_prediction(image_sizes, classnames, predictions, category_ids=None):
    """COCODetection.load_prediction (detnet/data/coco.py:229-252): normalised per-class [score,cx,cy,w,h] ->
    [{image_id, category_id, bbox [int x, y, w, h], score (5 decimals)}].  category ids default to 1..C
    (waymo_to_coco.py:19,36).  Dict form of export.detection_rows (kept for API parity)."""
    results = []
    for image_id, (width, height) in image_sizes.items():
        det = predictions[str(image_id)]
        scale = np.asarray([1, width, height, width, height])
        for cls, bbox in enumerate(det):
            bbox = bbox * scale
            bbox[:, 1:3] -= (bbox[:, 3:5] / 2)
            cat = category_ids[cls] if category_ids else cls + 1
            for box in bbox:
                results.append(dict(image_id=image_id, category_id=cat, bbox=[int(v) for v in box[1:5]],
                                    score=round(float(box[0]), 5)))
    return results


def list_images(root):
    root = Path(root)
    files = sorted(p for p in root.rglob('*') if p.suffix.lower() in IMG_EXT)
    return [(str(p.relative_to(root).with_suffix('')), p) for p in files]       # image_id = "<segment>/<ts>/<CAMERA>"


def autocontrast_(img_u8):
    """ImageOps.autocontrast(image) of PIL (cutoff 0; the reference's AutoContrast transform, trainer/transforms/vision.py:
    1069-1075) on a (H, W, 3) uint8 DEVICE tensor: per channel lo / hi = darkest / brightest value present; if hi <= lo the
    channel is unchanged, else lut[v] = clamp(int(v * 255 / (hi - lo) - lo * 255 / (hi - lo)), 0, 255).  Bit-exact with PIL
    (tests/test_gpu_detector.py); float64 like PIL's Python arithmetic."""
    if img_u8.is_cuda and img_u8.dim() == 3 and img_u8.shape[2] == 3:
        from .nn import ops
        return ops.autocontrast_(img_u8.contiguous().clone())          # two HIP launches; the torch formulation below is the CPU-tensor twin
    flat = img_u8.reshape(-1, img_u8.shape[-1])
    lo = flat.amin(0).double()
    hi = flat.amax(0).double()
    v = torch.arange(256, dtype=torch.float64, device=img_u8.device).unsqueeze(1)
    span = torch.where(hi > lo, hi - lo, torch.ones_like(hi))
    scale = torch.full_like(span, 255.0) / span          # true division: `255.0 / tensor` is reciprocal * 255 in torch (one ulp off PIL's scale)
    lut = torch.trunc(v * scale + (-lo * scale)).clamp_(0, 255)
    lut = torch.where((hi > lo).unsqueeze(0), lut, v.expand(-1, lut.shape[1])).to(torch.uint8)      # (256, C)
    out = torch.gather(lut, 0, flat.long())
    return out.reshape(img_u8.shape)


def resize_size(w, h, size, max_size=None):
    """Resize.compute_scaled_image_size (trainer/transforms/vision.py:168-190) for an int size: (out_h, out_w)."""
    if (w <= h and w == size) or (h <= w and h == size):
        return h, w
    if w < h:
        ow, oh = size, int(size * h / w)
    else:
        oh, ow = size, int(size * w / h)
    if max_size:
        if oh > max_size:
            ow, oh = int(max_size / oh * ow), max_size
        if ow > max_size:
            oh, ow = int(max_size / ow * oh), max_size
    return oh, ow


def parse_resize(args):
    """--resize as the reference parses it (detnet/inference.py:40): None, the length of the shorter edge (int), or for 'WxH' the
    pair (h, w) = reversed(s.split('x')), the exact output size.  A pair needs --resize-device gpu, and excludes --max-image-size as
    the reference's Resize asserts (vision.py:151-152)."""
    if args.resize is None:
        return None
    text = str(args.resize)
    if 'x' not in text:
        return int(text)
    if getattr(args, 'resize_device', 'host') != 'gpu':
        raise NotImplementedError('--resize WxH needs --resize-device gpu; on the host route --resize takes the length of the shorter edge (int)')
    try:
        size = tuple(int(item) for item in reversed(text.split('x')))
    except ValueError:
        size = ()
    if len(size) != 2:
        raise ValueError('--resize %r: WxH takes two integers' % text)
    if args.max_image_size:
        raise ValueError('--max-image-size only works with --resize <int>, not with a fixed WxH size')
    return size


class ImageLoader(object):
    """Decode ahead of the detector in a thread pool.  JPEG files: the file bytes go to the GPU and are decoded there
    (ops.jpeg_decode: Huffman, IDCT, upsampling, colour conversion in HIP kernels; bit-exact with PIL's decode, ~1 MB
    instead of 7.4 MB over PCIe per 1920x1280 frame).  Other formats: PIL decode + ToRGB, pinned staging buffer, asynchronous H2D
    of the uint8 HWC image.  Yields (image_id, device uint8 (H, W, 3), (width, height) of the ORIGINAL decoded image): the
    detector's boxes are normalised, and the reference's export scales them by the untransformed data set's image size
    (export.py:159-165 -> coco.py:243-246 with `dataset.dataset`), not by the resized one.

    Transform order of the reference (detnet/inference.py:170-178): ToRGB, AutoContrast, [CLAHE], Resize.  Without --resize
    AutoContrast runs on the GPU (autocontrast_, bit-exact with PIL); with --resize it has to precede the resize, so the loader
    applies it (`auto_contrast_in_loader`).  `resize` is the length of the shorter edge or an (h, w) pair; `resize_on` says where:
      'host' (default, the reference's way): every file is decoded by PIL, PIL's ImageOps.autocontrast and Image.resize(BILINEAR)
             run on the loader thread, the resized image is uploaded;
      'gpu':  the caller's `decoder` is kept - JPEG through ops.jpeg_decode, other files and the JPEG flavours the HIP decoder
             refuses through PIL and uploaded unresized - then ops.autocontrast_ and ops.resize_bilinear_u8 on the loader thread's
             stream (both bit-exact with PIL), and the thread synchronises that stream before it hands the frame over."""
    _warned = False                 # the PIL hand-over of an unsupported JPEG flavour is announced once


    def __init__(self, items, resize=None, max_image_size=None, workers=4, depth=4, auto_contrast=False, decoder='gpu', resize_on='host'):
        self.items, self.resize, self.max_size = items, resize, max_image_size
        self.workers, self.depth = workers, depth
        self.auto_contrast_in_loader = bool(auto_contrast and resize)
        assert decoder in ('gpu', 'pil') and resize_on in ('host', 'gpu')
        self.resize_on_gpu = bool(resize) and resize_on == 'gpu'
        if isinstance(resize, (tuple, list)):
            if not self.resize_on_gpu:
                raise NotImplementedError("an (h, w) resize needs resize_on='gpu'")
            if max_image_size:
                raise ValueError('max_image_size only works with an int resize')
        # JPEG files are decoded by the HIP decoder (csrc/jpeg_decode.hip, bit-exact with PIL) unless the image has to pass
        # through PIL's own resampling filter first (--resize on the host route: the reference resizes the PIL image, vision.py:137)
        # or the caller asks for the host decoder; other formats (PNG ...) are read by PIL as in the reference
        self.decoder = 'pil' if (resize and not self.resize_on_gpu) else decoder
        self._local = threading.local()

    def _out_size(self, w, h):
        if isinstance(self.resize, (tuple, list)):
            return int(self.resize[0]), int(self.resize[1])
        return resize_size(w, h, int(self.resize), self.max_size)

    def _stream(self):
        if getattr(self._local, 'stream', None) is None:
            self._local.stream = torch.cuda.Stream()                                # one stream per loader thread
        return self._local.stream

    def _decode_pil(self, path):
        from PIL import Image, ImageOps
        img = Image.open(path).convert('RGB')                                       # ToRGB (vision.py:954)
        size = img.size
        if self.resize_on_gpu:
            return np.asarray(img, dtype=np.uint8), size                            # AutoContrast and Resize follow on the device
        if self.auto_contrast_in_loader:
            img = ImageOps.autocontrast(img)                                        # AutoContrast precedes Resize
        if self.resize:
            oh, ow = self._out_size(img.width, img.height)
            img = img.resize((ow, oh), Image.BILINEAR)
        return np.asarray(img, dtype=np.uint8), size

    def _decode_file(self, path):
        if self.decoder == 'gpu':
            with open(path, 'rb') as f:
                data = f.read()
            if data[:2] == b'\xff\xd8':
                from .nn import ops
                try:
                    with torch.cuda.stream(self._stream()):
                        t = ops.jpeg_decode(data)                                   # returns with the image complete
                    return t, (t.shape[1], t.shape[0])
                except _lib.WaymoTrackError as e:
                    # a flavour the HIP decoder does not implement (progressive, CMYK, ...) is read the way PNG / BMP files are:
                    # by PIL, like the reference - said once, never silently; corrupt or truncated files still raise
                    if 'unsupported' not in str(e):
                        raise
                    if not ImageLoader._warned:
                        ImageLoader._warned = True
                        print('ImageLoader: %s: %s -> such files are decoded by PIL on the host' % (path, e), flush=True)
        return self._decode_pil(path)

    def _decode(self, path):
        t, size = self._decode_file(path)
        if not self.resize_on_gpu:
            return t, size
        from .nn import ops
        stream = self._stream()
        with torch.cuda.stream(stream):
            if isinstance(t, np.ndarray):
                t = torch.from_numpy(np.array(t, copy=True)).pin_memory().cuda(non_blocking=True)
            if self.auto_contrast_in_loader:
                t = ops.autocontrast_(t)                                            # in place: the decoded frame is the loader's own
            oh, ow = self._out_size(size[0], size[1])
            out = ops.resize_bilinear_u8(t, oh, ow)
        # the kernels above are asynchronous and the consumer only calls record_stream: the frame is complete before it leaves this
        # thread (which also keeps the pinned buffer and the decoded frame alive for as long as the stream reads them)
        stream.synchronize()
        return out, size

    def __iter__(self):
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(self.workers) as pool:
            pending = []
            it = iter(self.items)
            for image_id, path in it:
                pending.append((image_id, pool.submit(self._decode, path)))
                if len(pending) >= self.depth:
                    break
            while pending:
                image_id, fut = pending.pop(0)
                nxt = next(it, None)
                if nxt is not None:
                    pending.append((nxt[0], pool.submit(self._decode, nxt[1])))
                t, size = fut.result()
                if isinstance(t, np.ndarray):
                    t = torch.from_numpy(np.array(t, copy=True)).pin_memory().cuda(non_blocking=True)
                else:
                    t.record_stream(torch.cuda.current_stream())                    # allocated on a loader thread's stream
                yield image_id, t, size


def check_supported(args):
    """Flags of the reference that this path cannot honour fail loudly instead of being ignored."""
    if args.clahe:
        raise NotImplementedError('--clahe needs scikit-image equalize_adapthist (vision.py:1088-1092), which is not available')
    if args.device in ('cpu', 'half'):
        raise NotImplementedError('--device %s: the detector runs in fp32 on the GPU only (HIP kernels, no CPU fallback)' % args.device)
    if args.soft_nms or args.bbox_voting:
        raise NotImplementedError('--soft-nms / --bbox-voting belong to the SSD detect layer of the reference, not to Cascade R-CNN')
    parse_resize(args)
    if args.eval and not args.annotations:
        raise ValueError('--eval needs --annotations GT.json (COCO-format ground truth; the reference reads it from --data-root)')
    if getattr(args, 'eval_gpu', False) and not args.eval:
        raise ValueError('--eval-gpu selects how --eval scores the detections: give --eval --annotations GT.json with it')
    if args.export_format != 'json':
        raise NotImplementedError('--export-format json only')
    return check_views(args)


def run_rank(args, world, rank):
    """One process = one GPU: detect the shard, collate, and on rank 0 save / evaluate / export."""
    from . import nn as detnn
    from .trainer import Predictions
    from .. import distributed as D
    torch.backends.cudnn.benchmark = bool(args.cudnn_benchmark)
    if args.cudnn_benchmark:
        from ..tuning import enable_gemm_tuning
        enable_gemm_tuning()                       # library-GEMM counterpart of --cudnn-benchmark
    start = time.time()
    model = detnn.load(args.model).cuda().eval()
    tta = [t for t in args.tta.split(',') if t] if args.tta else None
    predict = PredictModel(model, dict(tta=tta, max_bbox=args.max_bbox))
    images = list_images(args.input)
    if args.exclusive:
        images = [(i, p) for i, p in images if args.exclusive not in i]
    image_ids = [i for i, _ in images]
    resumed = None
    if args.resume:                                # trainer/test.py:190-195: skip the samples already tested
        resumed = Predictions.open(args.resume)
        done = set(resumed.keys())
        if rank == 0:
            print(f"resuming {len(done)} tested samples")
        images = [(i, p) for i, p in images if i not in done]
    lo, hi = D.contiguous_split(len(images), world)[rank]
    store = Predictions(model.classnames, image_ids)
    sizes = np.zeros((len(image_ids), 2), np.int32)
    index = {k: i for i, k in enumerate(image_ids)}
    with torch.no_grad():
        loader = ImageLoader(images[lo:hi], parse_resize(args), args.max_image_size, auto_contrast=args.auto_contrast, decoder=args.decoder,
                             resize_on=args.resize_device)
        # round 6: `--inflight` detector passes in flight, each a captured hipGraph per image size (the Waymo cameras have two); results are collected
        # one image behind.  --inflight 0: the per-image eager call of the earlier rounds (and the only form for TTA plans / models without a
        # static-shape pass)
        lanes = predict.stream(args.inflight) if args.inflight > 0 else None
        pending = []
        for image_id, img, (w, h) in loader:
            if args.auto_contrast and not loader.auto_contrast_in_loader:
                img = autocontrast_(img)
            sizes[index[image_id]] = (w, h)
            if lanes is None:
                store[image_id] = predict(img.unsqueeze(0))[0]        # uint8 HWC -> fused pre-processing kernel
                continue
            if len(pending) >= args.inflight:                         # the oldest image's lane is the one this image will take
                k, t = pending.pop(0)
                store[k] = lanes[1](t)
            pending.append((image_id, lanes[0](img)))
        for k, t in pending:
            store[k] = lanes[1](t)
    cols, tested = store.shard_columns()
    allc = D.gather_columns_rank0(cols)                               # the one exchange: result rows -> rank 0
    meta = D.gather_columns_rank0(dict(image=np.nonzero(tested)[0].astype(np.int32), size=sizes[tested]))
    rows = None
    if rank == 0:
        mask = np.zeros(len(image_ids), bool)
        mask[meta['image']] = True
        sizes[meta['image']] = meta['size']
        predictions = Predictions.from_shards(model.classnames, image_ids, [allc], [mask])
        if resumed is not None:
            predictions.update(resumed)
        if args.output:                                              # trainer/test.py:272-276
            out_dir = Path(args.output)
            out_dir.mkdir(parents=True, exist_ok=True)
            print('saving', out_dir / 'detections.pkl')
            predictions.save(out_dir / 'detections.pkl')
        def image_sizes_in_order():
            """{image_id: (width, height)} of every tested image in data-set order (the reference iterates coco.imgs); resumed
            samples were not decoded in this run: their sizes come from the file headers."""
            out, paths = {}, None
            for i, k in enumerate(image_ids):
                if not predictions.tested[predictions._index[k]]:
                    continue
                if sizes[i, 0] > 0:
                    out[k] = (int(sizes[i, 0]), int(sizes[i, 1]))
                else:
                    from PIL import Image
                    paths = paths or dict(list_images(args.input))
                    with Image.open(paths[k]) as im:
                        out[k] = im.size
            return out
        image_sizes = image_sizes_in_order() if (args.eval or args.export) else {}
        if args.eval and getattr(args, 'eval_gpu', False):
            from .evaluate import evaluate_detection_sets
            for line in evaluate_detection_sets(args.annotations, [predictions])[0].lines():
                print(line)
        elif args.eval:
            from .data.metric import evaluate_detections
            evaluate_detections(predictions, args.annotations, image_sizes, print_fn=print)
        if args.export:
            from .export import export, detection_rows
            export(predictions, args.export, image_sizes, args.export_format, args.threshold)
            rows = detection_rows(predictions, image_sizes)
        print(f'inference done in {time.time() - start:.1f}s, {len(image_ids)} images, {len(allc["image"])} detections')
    return rows


def _spawned(rank, world, port, argv):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank))
    main(argv, _spawned_child=True)


def inference(args, argv=None):
    """detnet/inference.py:151-199 for an image folder."""
    views_spec = check_supported(args)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    if world == 1 and args.jobs > 1:                                  # -j N: one process per GPU (trainer/test.py:227-250)
        import socket
        import torch.multiprocessing as mp
        n_gpu = torch.cuda.device_count()
        if args.jobs > n_gpu:
            raise RuntimeError(f'-j {args.jobs} but only {n_gpu} GPUs are visible (one process per GPU)')
        with socket.socket() as sck:
            sck.bind(('127.0.0.1', 0))
            port = sck.getsockname()[1]
        mp.spawn(_spawned, args=(args.jobs, port, list(argv or [])), nprocs=args.jobs, join=True)
        return None
    if not torch.cuda.is_available():
        raise RuntimeError('the detector runs on the GPU only (HIP kernels, no CPU fallback)')
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
    if views_spec is not None:
        return run_views(args, views_spec)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group('nccl', device_id=torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0'))))
    try:
        rows = run_rank(args, world, rank)
    except BaseException:
        if world > 1:                                                 # no barrier here: the peers sit in a collective and a
            import torch.distributed as dist                         # barrier would mismatch it; tear the group down so they
            try:                                                     # fail fast instead of waiting for the RCCL timeout
                dist.destroy_process_group()
            except Exception:
                pass
        raise
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return rows


def main(argv=None, _spawned_child=False):
    import sys
    argv = list(sys.argv[1:] if argv is None else argv)
    args = build_parser().parse_args(argv)
    if not args.output and not args.eval and not args.export:
        raise UserWarning("Please specify at least one path for output / evaluation / export")
    return inference(args, argv)


if __name__ == '__main__':
    main()
