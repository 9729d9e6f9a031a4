"""ensemble submission with weighted boxes fusion / non-maximum weighted - drop-in for the reference's
detnet/ensemble_b.py (CLI flags, JSON formats).

``python -m waymo_2d_tracking_amd.detnet.ensemble_b A.json B.json -o OUT.json -m weighted_fusion --iou-thresh=0.5`` replaces
``python -m detnet.ensemble_b ...``.

The reference hands every image to the third-party ``ensemble_boxes`` package (ensemble_b.py:9,81-104).  Here the two merge rules
are the project's own definition - DESIGN.md section 17: the published weighted-boxes-fusion algorithm on the pixel corner boxes
ensemble_b.py:44-46 builds, with a defined order of equal scores and equal IoUs - and they are NOT pinned against that package.
``-m nms`` and ``-m soft_nms`` are the package's own NMS and Gaussian soft-NMS variants: not built, use ``detnet.ensemble``.

Data path: the input files are parsed by the native reader (ensemble.read_submission) into columns; the w > 0, h > 0 filter
(ensemble_b.py:65), the (image, category) grouping and each image's weight sum are column operations; every group of the whole
submission set is merged in ONE call of ``wt_fuse_groups_host`` (one wavefront per group, csrc/ensemble_wbf.hip); the merged rows
- sorted per image by score across the categories, float boxes, 5-decimal scores (ensemble_b.py:104-108) - are written by the
native JSON writer.  Under ``torchrun`` the images are split into contiguous blocks like detnet.ensemble.
"""
import argparse
import ctypes as C
import math
import os
from pathlib import Path

import numpy as np

from .. import _lib
from . import ensemble as E

METHODS = {'weighted_fusion': 0, 'nmw': 1}
CLI_METHODS = ("weighted_fusion", "nms", "soft_nms", "nmw")


def check_method(method):
    if method in ('nms', 'soft_nms'):
        raise NotImplementedError("-m %s of ensemble_b is the ensemble_boxes package's own variant and is not built: use "
                                  "waymo_2d_tracking_amd.detnet.ensemble -m %s" % (method, method))
    if method not in METHODS:
        raise ValueError('unknown ensemble_b method %r' % (method,))
    return METHODS[method]


def input_weights(weights, k):
    """Per-input weights as given (the package does not normalise them); None = all 1."""
    w = [1.0] * k if weights is None else [float(v) for v in weights]
    if len(w) != k:
        raise ValueError('%d weights for %d inputs' % (len(w), k))
    if not all(math.isfinite(v) and v > 0 for v in w):
        raise ValueError('weights must be positive and finite, got %s' % w)
    return w


def merge_inputs(subs, weights=None):
    """convert_submission (ensemble_b.py:54-70) on columns.  Returns (image_ids, category_ids, rows, image_wsum): rows as
    ensemble.merge_inputs gives them (w > 0 and h > 0 kept, score already multiplied by its input's weight, images in
    first-appearance order) and, per image, the weight sum of the inputs that kept a row of any category in it (ensemble_b.py:96-101
    passes only those inputs to the merge), added in input order.  Non-finite scores or coordinates are a ValueError."""
    w = input_weights(weights, len(subs))
    for k, s in enumerate(subs):
        for c in ('score', 'x', 'y', 'w', 'h'):
            bad = ~np.isfinite(np.asarray(s[c], np.float64))
            if bad.any():
                i = int(np.argmax(bad))
                raise ValueError('input %d, row %d (image %s): %s is %r' % (k, i, s['image_ids'][int(s['image'][i])], c, float(s[c][i])))
    image_ids, category_ids, rows = E.merge_inputs(subs, w, -math.inf)
    present = np.zeros((len(image_ids), len(subs)), bool)
    present[rows['image'].astype(np.int64), rows['input'].astype(np.int64)] = True
    wsum = np.zeros(len(image_ids), np.float64)
    for k in range(len(subs)):
        wsum = wsum + np.where(present[:, k], w[k], 0.0)
    return image_ids, category_ids, rows, wsum


def pack_groups(n_images, category_ids, rows, k_inputs, image_wsum, image_lo=0, image_hi=None):
    """ensemble.pack_groups plus group_wsum: every (image, category) group carries its image's weight sum."""
    packed = E.pack_groups(n_images, category_ids, rows, k_inputs, image_lo, image_hi)
    hi = n_images if image_hi is None else image_hi
    packed['group_wsum'] = np.ascontiguousarray(np.repeat(np.asarray(image_wsum, np.float64)[image_lo:hi], packed['ncat']))
    return packed


def merge_groups(packed, method, iou_thresh):
    """wt_fuse_groups_host on one packed block -> (out5, counts, members, row_cluster)."""
    code = check_method(method)
    d = packed['dets5']
    G = packed['n_groups']
    out5 = np.zeros((len(d) + 1, 5), dtype=np.float64)
    members = np.zeros(len(d) + 1, dtype=np.int32)
    row_cluster = np.zeros(len(d) + 1, dtype=np.int32)
    counts = np.zeros(G + 1, dtype=np.int64)
    if G:
        rc = _lib.lib().wt_fuse_groups_host(
            _lib.ptr(d), _lib.ptr(packed['group_offsets']), _lib.ptr(packed['group_wsum']), C.c_int64(G), C.c_int(code),
            C.c_double(iou_thresh), _lib.ptr(out5), _lib.ptr(members), _lib.ptr(row_cluster), _lib.ptr(counts))
        _lib.check(rc, 'wt_fuse_groups_host')
    return out5[:len(d)], counts[:G], members[:len(d)], row_cluster[:len(d)]


def output_rows(packed, category_ids, out5, counts):
    """ensemble_b.py:104-108 on columns: per image the merged rows of all its categories by descending score (equal scores:
    ascending category, then the group's own order), bbox as floats [x, y, w, h], round(score, 5)."""
    off = packed['group_offsets'][:-1]
    G = packed['n_groups']
    counts = np.asarray(counts, np.int64)
    idx = np.concatenate([np.arange(o, o + c) for o, c in zip(off.tolist(), counts.tolist())]) if G and counts.sum() else np.zeros(0, np.int64)
    group = np.repeat(np.arange(G), counts)
    image = group // packed['ncat'] + packed['image_lo'] if len(group) else np.zeros(0, np.int64)
    s = out5[idx, 0]
    order = np.lexsort((-s, image))                    # stable: rows are in (category, group order) inside an image
    idx, group, image, s = idx[order], group[order], image[order], s[order]
    score = np.asarray([round(v, 5) for v in s.tolist()], dtype=np.float64)
    cats = np.asarray(category_ids, np.int32)
    return dict(image=image.astype(np.int32), category=cats[group % packed['ncat']] if len(group) else np.zeros(0, np.int32),
                bbox=np.ascontiguousarray(out5[idx, 1:5], dtype=np.float64).reshape(-1, 4), score=score)


def fuse_columns(image_ids, category_ids, rows, k_inputs, image_wsum, method='weighted_fusion', iou_thresh=0.5, merge_fn=None):
    """All groups -> output columns; with torch.distributed initialised every rank merges the groups of its contiguous block of
    images and rank 0 receives all rows (None elsewhere).  merge_fn(packed, method, iou_thresh) -> (out5, counts, ...) replaces the
    HIP call (tests: the restatement)."""
    from .. import distributed as D
    check_method(method)
    w, r = D.world()
    lo, hi = D.contiguous_split(len(image_ids), w)[r]
    packed = pack_groups(len(image_ids), category_ids, rows, k_inputs, image_wsum, lo, hi)
    out5, counts = (merge_fn or merge_groups)(packed, method, iou_thresh)[:2]
    return D.gather_columns_rank0(output_rows(packed, category_ids, out5, counts))


def fuse_submissions(subs, method='weighted_fusion', iou_thresh=0.5, weights=None, merge_fn=None):
    """Parsed inputs (columns of ensemble.read_submission / submission_columns) -> (image_ids, output columns)."""
    image_ids, category_ids, rows, wsum = merge_inputs(subs, weights)
    return image_ids, fuse_columns(image_ids, category_ids, rows, len(subs), wsum, method, iou_thresh, merge_fn)


def write_detections_json(path, image_ids, rows):
    """json.dump([{image_id, category_id, bbox, score}, ...]) of column rows with float boxes through libwaymotrack."""
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    blobs = [str(s).encode('utf-8') for s in image_ids]
    offsets = np.zeros(len(blobs) + 1, np.int64)
    np.cumsum([len(b) for b in blobs], out=offsets[1:])
    blob = b''.join(blobs) or b'\0'
    img = np.ascontiguousarray(rows['image'], dtype=np.int32)
    cat = np.ascontiguousarray(rows['category'], dtype=np.int32)
    bbox = np.ascontiguousarray(rows['bbox'], dtype=np.float64).reshape(-1, 4)
    score = np.ascontiguousarray(rows['score'], dtype=np.float64)
    rc = _lib.lib().wt_detections_write_json_f64(str(path).encode(), C.c_int64(len(img)), _lib.ptr(img), C.c_int32(len(blobs)),
                                                 C.c_char_p(blob), _lib.ptr(offsets), _lib.ptr(cat), _lib.ptr(bbox), _lib.ptr(score))
    _lib.check(rc, 'wt_detections_write_json_f64')


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter,
                                     fromfile_prefix_chars='@')
    parser.add_argument('inputs', type=str, nargs='+', help='input json files')
    parser.add_argument('-o', '--output', type=str, help='output json file')
    parser.add_argument('-m', '--method', choices=CLI_METHODS, default="weighted_fusion", help='method to merge bbox detections')
    parser.add_argument('--iou-thresh', type=float, default=0.5, help='IOU threshold for merging bboxes')
    return parser


def main(argv=None, merge_fn=None):
    args = build_parser().parse_args(argv)
    check_method(args.method)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))

    input_files = []
    for f in args.inputs:
        f = Path(f)
        if f.is_file():
            input_files.append(f)
        elif f.is_dir():
            input_files += sorted(f.glob("**/*.json"))     # the reference takes glob order, which the file system decides
        else:
            print(f"{f} is neither file nor dir?!")
    assert len(input_files) > 1
    if rank == 0:
        print('input files:', input_files)

    output_file = Path(args.output)
    output_file.parent.mkdir(parents=True, exist_ok=True)
    if output_file.exists():
        raise RuntimeError(f"output file {output_file} exists!")

    if world > 1:
        import torch
        import torch.distributed as dist
        backend = os.environ.get('WT_DIST_BACKEND', 'nccl')
        if backend == 'nccl':
            torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
        dist.init_process_group(backend)
    subs = [E.read_submission(f) for f in input_files]
    image_ids, category_ids, rows, wsum = merge_inputs(subs)
    if rank == 0:
        print('No. Images:', len(image_ids))
        print('No. categories:', len(category_ids))
    out = fuse_columns(image_ids, category_ids, rows, len(subs), wsum, args.method, args.iou_thresh, merge_fn)
    if rank == 0:
        write_detections_json(output_file, image_ids, out)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
