"""Host side of detnet/ensemble_b.py without a GPU: command line, refusals, grouping and weight sums, the per-image output order
and the float-box JSON writer.  The merge itself is tests/wbf_ref.py through `merge_fn`; the kernel is in tests/test_gpu_wbf.py."""
import json

import numpy as np
import pytest

import wbf_ref as R


def _row(image, category, score, bbox):
    return {'image_id': image, 'category_id': category, 'bbox': bbox, 'score': score}


A = [_row('p', 1, 0.75, [0, 0, 10, 10]), _row('p', 2, 0.5, [40, 40, 10, 10]), _row('q', 1, 0.5, [0, 0, 4, 4])]
B = [_row('p', 1, 0.25, [2, 0, 10, 10]), _row('q', 1, 0.9, [0, 0, 0, 4])]          # the q row has zero width: dropped
C = [_row('p', 2, 0.25, [40, 40, 10, 10])]                                        # image q is missing here


def _write(tmp_path, subs):
    paths = []
    for k, rows in enumerate(subs):
        paths.append(str(tmp_path / ('in%d.json' % k)))
        with open(paths[-1], 'w') as fp:
            json.dump(rows, fp)
    return paths


def test_parser_is_the_reference_command_line():
    from waymo_2d_tracking_amd.detnet import ensemble_b as EB
    args = EB.build_parser().parse_args(['A.json', 'B.json', '-o', 'O.json'])
    assert args.inputs == ['A.json', 'B.json'] and args.output == 'O.json' and args.method == 'weighted_fusion' and args.iou_thresh == 0.5
    args = EB.build_parser().parse_args(['d', 'e', '--output', 'O.json', '-m', 'nmw', '--iou-thresh', '0.55'])
    assert args.method == 'nmw' and args.iou_thresh == 0.55
    for m in ('weighted_fusion', 'nms', 'soft_nms', 'nmw'):
        assert EB.build_parser().parse_args(['a', 'b', '-o', 'o', '-m', m]).method == m
    with pytest.raises(SystemExit):
        EB.build_parser().parse_args(['a', 'b', '-o', 'o', '-m', 'average'])


def test_refusals(tmp_path):
    from waymo_2d_tracking_amd.detnet import ensemble_b as EB
    paths = _write(tmp_path, [A, B])
    for m in ('nms', 'soft_nms'):
        with pytest.raises(NotImplementedError, match=r'detnet\.ensemble '):
            EB.main(paths + ['-o', str(tmp_path / 'never.json'), '-m', m], merge_fn=R.merge_fn)
        with pytest.raises(NotImplementedError):
            EB.fuse_submissions([EB.E.submission_columns(A), EB.E.submission_columns(B)], m, 0.5, merge_fn=R.merge_fn)
    assert not (tmp_path / 'never.json').exists()
    existing = tmp_path / 'there.json'
    existing.write_text('[]')
    with pytest.raises(RuntimeError, match='exists'):
        EB.main(paths + ['-o', str(existing)], merge_fn=R.merge_fn)
    assert existing.read_text() == '[]'
    with pytest.raises(AssertionError):
        EB.main(paths[:1] + ['-o', str(tmp_path / 'one.json')], merge_fn=R.merge_fn)
    for bad in (_row('p', 1, float('nan'), [0, 0, 1, 1]), _row('p', 1, 0.5, [0, float('inf'), 1, 1]), _row('p', 1, 0.5, [0, 0, -float('inf'), 1])):
        with pytest.raises(ValueError):
            EB.fuse_submissions([EB.E.submission_columns(A), EB.E.submission_columns([bad])], merge_fn=R.merge_fn)
    with pytest.raises(ValueError):
        EB.fuse_submissions([EB.E.submission_columns(A), EB.E.submission_columns(B)], weights=[1, 0], merge_fn=R.merge_fn)
    with pytest.raises(ValueError):
        EB.fuse_submissions([EB.E.submission_columns(A), EB.E.submission_columns(B)], 'average', merge_fn=R.merge_fn)


def test_grouping_and_wsum_of_three_inputs():
    from waymo_2d_tracking_amd.detnet import ensemble_b as EB
    subs = [EB.E.submission_columns(s) for s in (A, B, C)]
    image_ids, category_ids, rows, wsum = EB.merge_inputs(subs)
    assert image_ids == ['p', 'q'] and category_ids == [1, 2]
    assert wsum.tolist() == [3.0, 1.0]                       # p: all three inputs (C only in category 2); q: A alone
    packed = EB.pack_groups(2, category_ids, rows, 3, wsum)
    assert packed['group_offsets'].tolist() == [0, 2, 4, 5, 5]                  # (p,1) (p,2) (q,1) (q,2)
    assert packed['group_wsum'].tolist() == [3.0, 3.0, 1.0, 1.0]
    assert packed['dets5'].tolist() == [[0.75, 0, 0, 10, 10], [0.25, 2, 0, 10, 10], [0.5, 40, 40, 10, 10], [0.25, 40, 40, 10, 10], [0.5, 0, 0, 4, 4]]
    image_ids, out = EB.fuse_submissions(subs, merge_fn=R.merge_fn)
    assert out['image'].tolist() == [0, 0, 1] and out['category'].tolist() == [1, 2, 1]
    assert out['score'].tolist() == [0.33333, 0.25, 0.5]
    assert out['bbox'].dtype == np.float64 and out['bbox'].tolist() == [[0.5, 0, 10, 10], [40, 40, 10, 10], [0, 0, 4, 4]]
    # explicit weights multiply the scores and make up wsum
    _, _, rows, wsum = EB.merge_inputs(subs, [2, 1, 0.5])
    assert wsum.tolist() == [3.5, 2.0] and rows['score'].tolist() == [1.5, 1.0, 1.0, 0.25, 0.125]


def test_rows_of_an_image_are_sorted_across_categories():
    from waymo_2d_tracking_amd.detnet import ensemble_b as EB
    a = [_row('r', 2, 0.5, [0, 0, 8, 8]), _row('r', 1, 0.5, [0, 0, 8, 8]), _row('r', 1, 0.75, [100, 0, 8, 8]), _row('r', 3, 0.625, [0, 0, 8, 8]),
         _row('s', 3, 0.25, [0, 0, 8, 8])]
    b = [_row('t', 1, 0.5, [0, 0, 8, 8]), _row('s', 1, 0.125, [0, 0, 8, 8])]
    image_ids, out = EB.fuse_submissions([EB.E.submission_columns(a), EB.E.submission_columns(b)], 'nmw', 0.5, merge_fn=R.merge_fn)
    assert image_ids == ['r', 's', 't']                     # first appearance, input by input
    assert list(zip(out['image'].tolist(), out['category'].tolist(), out['score'].tolist())) == [
        (0, 1, 0.75), (0, 3, 0.625), (0, 1, 0.5), (0, 2, 0.5), (1, 3, 0.25), (1, 1, 0.125), (2, 1, 0.5)]


def test_host_path_equals_the_restatement_of_the_whole_file_flow(tmp_path):
    from waymo_2d_tracking_amd import synthetic as syn
    from waymo_2d_tracking_amd.detnet import ensemble_b as EB
    subs = syn.ensemble_inputs_json(5, n_images=4, k_inputs=3, n_objects=12)
    subs[2] = [r for r in subs[2] if r['image_id'] != subs[0][0]['image_id']]          # one image missing from one input
    paths = _write(tmp_path, subs)
    for method, thr in (('weighted_fusion', 0.5), ('nmw', 0.6)):
        out = tmp_path / ('out_%s.json' % method)
        EB.main(paths + ['-o', str(out), '-m', method, '--iou-thresh', str(thr)], merge_fn=R.merge_fn)
        exp = R.ensemble_rows(subs, method, thr)
        assert len(exp) > 8 and json.load(open(out)) == exp
        assert out.read_text() == json.dumps(exp)


def test_float_box_writer_equals_json_dump_byte_for_byte(tmp_path):
    from waymo_2d_tracking_amd.detnet import ensemble_b as EB
    values = [0.1 + 0.2, 1e-7, 1e16, 1e22, -0.0, 123456789.125, 5e-324, 1.7976931348623157e308, 40.0, 1 / 3, 2.5e-5, 9999999999999998.0,
              1e15 + 0.5, 0.0001, 0.00001, 1234.5678, -17.25, 2.0 ** 53, 1e21, 123456789012345680.0]
    bbox = np.asarray(values, np.float64).reshape(-1, 4)
    n = len(bbox)
    image_ids = ['seg/0/FRONT', 'café "x"\\y', '\U0001f600']
    rows = dict(image=np.arange(n) % 3, category=np.arange(n) % 4 + 1, bbox=bbox, score=np.asarray([round(0.1 * (i + 1) / 3, 5) for i in range(n)]))
    path = tmp_path / 'sub' / 'f.json'
    EB.write_detections_json(path, image_ids, rows)
    exp = [{'image_id': image_ids[i % 3], 'category_id': i % 4 + 1, 'bbox': bbox[i].tolist(), 'score': float(rows['score'][i])} for i in range(n)]
    assert path.read_bytes() == json.dumps(exp).encode()
    EB.write_detections_json(tmp_path / 'empty.json', image_ids, dict(image=np.zeros(0, np.int32), category=np.zeros(0, np.int32),
                                                                      bbox=np.zeros((0, 4)), score=np.zeros(0)))
    assert (tmp_path / 'empty.json').read_text() == '[]'
