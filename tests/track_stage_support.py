"""What the GPU tests of the six track post-passes (tests/test_gpu_track_{refine,stitch,smooth,dedup,split,xclass}.py, DESIGN.md
sections 20-26) share: the hand-made input forms, the tracked fixtures, the chain of reference passes, one comparator per stage and
the bodies of the tests that are the same for every stage.  A stage's file calls a body with its STAGES entry and keeps what is its
own.

This module is not rewritten by pytest: every assert carries the field or the stage it compared as its message."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest

import dedup_ref
import hota_ref
import mot_id_ref
import mot_ref
import refine_ref
import smooth_ref
import split_ref
import stitch_ref
import xclass_ref
from track_cases import N_CLASSES

G4 = dict(score=[0.3, 0.3, 1.0, 0.2], iou=[0.01, 0.01, 1.0, 0.0])
G5 = dict(score=[0.95, 0.6, 1.0, 0.9], iou=[0.01, 0.01, 1.0, 0.0])
COLUMNS = ('frame', 'category', 'bbox', 'score', 'object_id')
ORDER = ('split', 'stitch', 'dedup', 'xclass', 'refine', 'smooth')      # of tracking.track.PASSES


def packed_for(offsets):
    """the part of a packed detection set that the passes read, for hand-made slots"""
    offsets = np.asarray(offsets, np.int64)
    n_streams = offsets.size - 1
    ids = np.concatenate([np.arange(offsets[s + 1] - offsets[s]) * 10 + 5 for s in range(n_streams)] + [np.zeros(0, np.int64)])
    return {'stream_frame_offsets': offsets, 'frame_ids': ids.astype(np.int64), 'stream_keys': [('seg%d' % s, 'FRONT') for s in range(n_streams)]}


def arrays(result, id_dtype=np.int64):
    """the five columns of a hand-made result or of a reference's output as the arrays the passes and the writers take"""
    return {'frame': np.asarray(result['frame'], np.int64), 'category': np.asarray(result['category'], np.int32),
            'bbox': np.asarray(result['bbox'], np.float64).reshape(-1, 4), 'score': np.asarray(result['score'], np.float64),
            'object_id': np.asarray(result['object_id'], id_dtype)}


def with_ids(out, ref):
    """the input rows with the reference's object ids: what the later passes and the writers take"""
    return dict(out, object_id=np.asarray(ref['object_id'], dtype=np.asarray(out['object_id']).dtype))


def with_boxes(out, ref):
    """the input rows with the reference's boxes: what the writers take"""
    return dict(out, bbox=np.asarray(ref['bbox'], np.float64).reshape(-1, 4))


def gt_box(o, f):
    """object o at slot f, linear in the slot with steps divisible by 4 (the stitch and the smooth effect tests)"""
    return [100.0 * o + 8.0 * f, 50.0 + 4.0 * f, 40.0, 30.0]


def same_bits(got, ref):
    """got, a float64 array, equals ref - anything of its shape - bit for bit, any NaN equal to any NaN: -0.0 is not 0.0, and a got of
    another dtype or shape equals nothing"""
    ref = np.ascontiguousarray(ref, np.float64)
    if not (isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == ref.shape):
        return False
    got = np.ascontiguousarray(got)
    return bool(((got.view(np.int64) == ref.view(np.int64)) | (np.isnan(got) & np.isnan(ref))).all())


def predictions_of(dets):
    """a detection list as predictions[seg][cam][frame], the form utils.pack_streams takes"""
    predictions = {}
    for e in dets:
        seg, fr, cam = e['image_id'].split('/')
        predictions.setdefault(seg, {}).setdefault(cam, {}).setdefault(int(fr), []).append(
            {'bbox': e['bbox'], 'score': e['score'], 'category_id': e['category_id']})
    return predictions


def lds_limit(stage):
    """the trajectory count up to which the stage keeps its tables in LDS"""
    from waymo_2d_tracking_amd import _lib
    n = C.c_int32(0)
    getattr(_lib.lib(), 'wt_%s_tracks_limits' % stage)(C.byref(n))
    return n.value


def tracked_fixtures(golden_dir):
    """The two tracking fixtures tracked with max_age 2 (a track ends at its third miss): [(packed, out)], g4 first."""
    from waymo_2d_tracking_amd.tracking import utils as T
    sets = []
    for name, cfg in (('sort_g4_input.json', G4), ('sort_g5_input.json', G5)):
        packed = T.pack_streams(T.read_data_file(os.path.join(golden_dir, name), cfg['score']))
        sets.append((packed, T.track_packed(packed, cfg['iou'], 2, 0)[0]))
    return sets


def without_frames(dets, picks):
    """the detections without classes 1 and 2 in the frames at the positions `picks` of the sorted frame list"""
    frames = sorted(set(int(e['image_id'].split('/')[1]) for e in dets))
    drop = set(frames[i] for i in picks)
    return [e for e in dets if not (int(e['image_id'].split('/')[1]) in drop and e['category_id'] != 4)]


def sweep_set(tmp_path_factory, name, n_frames=12, edit=None):
    """synthetic detections of one segment and two cameras, `edit`ed, in a file: (path, dets, gt_json)"""
    from waymo_2d_tracking_amd import synthetic as syn
    dets, gt_json = syn.make_tracking_json(23, n_segments=1, n_frames=n_frames, n_objects=12, cameras=('FRONT', 'SIDE_LEFT'))
    if edit is not None:
        dets = edit(dets)
    path = tmp_path_factory.mktemp(name) / 'det.json'
    path.write_text(json.dumps(dets))
    return str(path), dets, gt_json


# ---- one comparator per stage: got is a dict of tracking/<stage>.py, ref the reference's output for the rows `out` ----

def _equal(got, want, name):
    assert got.tolist() == want, name


def _untouched(got, out, names):
    for name in names:                                                    # no row is added, removed, moved or changed
        assert got[name].dtype == np.asarray(out[name]).dtype and got[name].tobytes() == np.asarray(out[name]).tobytes(), name


def assert_same_refine(got, ref, out=None):
    for name in ('frame', 'source', 'category', 'frame_row_offsets'):
        _equal(got[name], ref[name], name)
    assert [int(v) for v in got['object_id']] == ref['object_id'], 'object_id'
    assert got['bbox'].dtype == np.float64 and got['score'].dtype == np.float64, 'bbox / score dtype'
    assert got['bbox'].tobytes() == np.asarray(ref['bbox'], np.float64).reshape(-1, 4).tobytes(), 'bbox'
    assert got['score'].tobytes() == np.asarray(ref['score'], np.float64).tobytes(), 'score'


def assert_same_stitch(got, ref, out):
    assert [int(v) for v in got['object_id']] == ref['object_id'], 'object_id'
    for name in ('pred', 'root', 'row_root', 'n_links', 'traj_offsets'):
        _equal(got[name], ref[name], name)
    assert got['affinity'].dtype == np.float64 and got['affinity'].tobytes() == np.asarray(ref['affinity'], np.float64).tobytes(), 'affinity'
    assert [(f, t, n, a) for f, t, n, a in got['links']] == ref['links'], 'links'
    _untouched(got, out, ('frame', 'category', 'bbox', 'score'))
    assert got['object_id'].dtype == np.asarray(out['object_id']).dtype, 'object_id dtype'


def assert_same_smooth(got, ref, out):
    assert got['bbox'].dtype == np.float64 and got['bbox'].shape == (len(ref['bbox']), 4), 'bbox dtype / shape'
    assert same_bits(got['bbox'], np.asarray(ref['bbox'], np.float64).reshape(-1, 4)), 'bbox'
    assert got['pairs'].dtype == np.int32 and got['pairs'].tolist() == ref['pairs'], 'pairs'
    _untouched(got, out, ('frame', 'category', 'score', 'object_id'))


def _assert_same_survivors(got, ref, out):
    """what dedup and xclass share: the decisions, and the surviving rows, in the caller's order, with their input bits"""
    for name in ('keep', 'by', 'match', 'row_keep', 'n_dropped', 'traj_offsets'):
        _equal(got[name], ref[name], name)
    assert [(int(a), int(b), m) for a, b, m in got['dropped']] == ref['dropped'], 'dropped'
    mask = np.asarray(ref['row_keep'], bool)
    for name in COLUMNS:
        want = np.asarray(out[name])[mask]
        assert got[name].dtype == want.dtype and got[name].shape == want.shape and got[name].tobytes() == want.tobytes(), name
    assert [int(v) for v in got['frame']] == ref['frame'] and [int(v) for v in got['object_id']] == ref['object_id'], 'frame / object_id'


def assert_same_dedup(got, ref, out):
    _assert_same_survivors(got, ref, out)
    assert got['bbox'].tobytes() == np.asarray(ref['bbox'], np.float64).reshape(-1, 4).tobytes(), 'bbox'
    assert got['score'].tobytes() == np.asarray(ref['score'], np.float64).tobytes(), 'score'


assert_same_xclass = _assert_same_survivors


def assert_same_split(got, ref, out):
    assert [int(v) for v in got['object_id']] == ref['object_id'], 'object_id'
    assert got['piece'].dtype == np.int32 and got['piece'].tolist() == ref['piece'], 'piece'
    assert got['new'].dtype == np.int64 and got['new'].tolist() == ref['new'], 'new'
    assert got['test'].shape == (len(ref['test']), 2) and same_bits(got['test'], np.asarray(ref['test'], np.float64).reshape(-1, 2)), 'test'
    assert got['breaks'].dtype == np.int32 and got['breaks'].tolist() == ref['breaks'], 'breaks'
    for name in ('n_new_pieces', 'traj_offsets'):
        _equal(got[name], ref[name], name)
    assert got['n_new'] == ref['n_new'], 'n_new'
    _untouched(got, out, ('frame', 'category', 'bbox', 'score'))
    assert got['object_id'].dtype == np.asarray(out['object_id']).dtype, 'object_id dtype'


class Stage:
    """One post-pass: its library module, entry points and cases (looked up when first used - the library needs a GPU to run), its
    reference, its comparator and how the reference's output becomes the next pass's input rows."""

    def __init__(self, name, device, reference, assert_same, rows):
        self.name, self._device, self.reference, self.assert_same, self.rows = name, device, reference, assert_same, rows

    module = property(lambda self: importlib.import_module('waymo_2d_tracking_amd.tracking.' + self.name))
    tracks = property(lambda self: getattr(self.module, self.name + '_tracks'))
    device = property(lambda self: getattr(self.module, self._device))
    cases = property(lambda self: importlib.import_module(self.name + '_cases'))


STAGES = dict((s.name, s) for s in (
    Stage('split', 'DeviceSplit', split_ref.split, assert_same_split, with_ids),
    Stage('stitch', 'DeviceStitch', stitch_ref.stitch, assert_same_stitch, with_ids),
    Stage('dedup', 'DeviceDedup', dedup_ref.dedup, assert_same_dedup, lambda out, ref: arrays(ref)),
    Stage('xclass', 'DeviceXClass', lambda offsets, result, job: xclass_ref.xclass(offsets, result, job, N_CLASSES), assert_same_xclass,
          lambda out, ref: arrays(ref)),
    Stage('refine', 'DeviceRefine', refine_ref.refine, assert_same_refine, lambda out, ref: arrays(ref)),
    Stage('smooth', 'DeviceSmooth', smooth_ref.smooth, assert_same_smooth, with_boxes)))


# ---- the reference chain ----

def reference_passes(packed, out, passes):
    """The rows `out` through the reference passes {stage: job} (or (stage, job) pairs), in the fixed order of tracking.track.PASSES
    whatever order they are given in: (the rows the writers take, {stage: that reference's output})."""
    passes = dict(passes)
    assert set(passes) <= set(ORDER), sorted(passes)
    rows, refs = dict((k, out[k]) for k in COLUMNS), {}
    for name in ORDER:
        if name in passes:
            refs[name] = STAGES[name].reference(packed['stream_frame_offsets'], rows, passes[name])
            rows = STAGES[name].rows(rows, refs[name])
    return rows, refs


def _expected_file(path, score_thr, iou_thr, max_age, passes):
    """What track.py has to write: the tracker's rows through the reference passes and format_tracks; the new ids of a split from
    the id counter.  Returns (the rows of the file, {stage: reference output}, the tracker's rows, its births)."""
    from waymo_2d_tracking_amd.tracking import utils as T
    packed = T.pack_streams(T.read_data_file(path, score_thr))
    out, births = T.track_packed(packed, iou_thr, max_age, 0)
    passes = dict(passes)
    if 'split' in passes:
        passes['split'] = dict(passes['split'], first_new_id=births + 1)     # a birth is written as the counter + 1
    rows, refs = reference_passes(packed, out, passes)
    return T.format_tracks(packed, rows), refs, out, births


METRIC_REFS = {'mot': lambda gt, rows: mot_ref.evaluate(gt, rows)['table'], 'id': lambda gt, rows: mot_id_ref.evaluate(gt, rows)['table'],
               'hota': hota_ref.evaluate}


def sweep_reference(dets, gt_json, passes_of, metrics=('mot', 'id', 'hota')):
    """reference(s): what the restatements give for one setting s of a sweep - the detections tracked under s (once per tracker
    setting), through the reference passes passes_of(s), written and read like a file, under each of `metrics`; computed once."""
    from waymo_2d_tracking_amd.tracking import utils as T
    packed = T.pack_streams(predictions_of(dets))
    cache, tracked = {}, {}

    def reference(s):
        key = tuple(sorted(s.items()))
        if key not in cache:
            tkey = (s['iou'], s['max_age'], s['min_hits'], s['score'])
            if tkey not in tracked:
                tracked[tkey] = T.track_packed(packed, [s['iou']] * 4, s['max_age'], s['min_hits'], [s['score']] * 4)[0]
            rows = json.loads(json.dumps(T.format_tracks(packed, reference_passes(packed, tracked[tkey], passes_of(s))[0])))
            cache[key] = tuple(METRIC_REFS[m](gt_json, rows) for m in metrics)
        return cache[key]
    return reference


# ---- the test bodies that are the same for every stage ----

def check_case(stage, name, run=None):
    """test_case_equals_reference: the case is in its class by the reference alone, and the host form (or `run`) equals it"""
    offsets, result, jobs, claim = stage.cases.CASES[name]()
    refs = [stage.reference(offsets, result, j) for j in jobs]
    claim(refs)
    out = arrays(result)
    got = run(offsets, result, jobs) if run is not None else stage.tracks(packed_for(offsets), [out], jobs)
    assert len(got) == len(refs), (stage.name, name, len(got), len(refs))
    for g, ref in zip(got, refs):
        stage.assert_same(g, ref, out)


def check_either_side_of_the_lds_limit(stage, above, make_case=None):
    """test_trajectory_counts_on_either_side_of_the_lds_limit: limit + above trajectories in one stream, host and device form"""
    limit = lds_limit(stage.name)
    assert 64 < limit <= 4096, (stage.name, limit)
    offsets, result, jobs, claim = (make_case or stage.cases.many_trajectories)(limit + above)
    refs = [stage.reference(offsets, result, j) for j in jobs]
    claim(refs)
    out = arrays(result)
    p = stage.module._prepare(packed_for(offsets), [out], jobs, N_CLASSES)
    assert p['n_traj'].tolist() == [[limit + above]], (stage.name, p['n_traj'].tolist())
    for g, ref in zip(stage.tracks(packed_for(offsets), [out], jobs), refs):
        stage.assert_same(g, ref, out)
    dev = stage.device(packed_for(offsets), [out], jobs)
    dev.launch()
    for g, ref in zip(dev.results(), refs):
        stage.assert_same(g, ref, out)


def check_jobs_over_results(stage, packed, outs, refs, settings, pairs):
    """The first part of test_jobs_over_results_in_one_call_equal_single_calls_and_dev_equals_host: the jobs settings[j] on
    outs[r] for the (r, j) of `pairs` in one host call, in one device call and alone all equal refs[r][j].  Returns the device
    form, launched, its jobs and its results."""
    jobs = [dict(settings[j], result=r) for r, j in pairs]
    together = stage.tracks(packed, outs, jobs)
    dev = stage.device(packed, outs, jobs)
    dev.launch()
    from_dev = dev.results()
    assert len(together) == len(from_dev) == len(pairs), (stage.name, len(together), len(from_dev))
    for (r, j), a, b in zip(pairs, together, from_dev):
        alone = stage.tracks(packed, [outs[r]], [settings[j]])[0]
        for got in (alone, a, b):
            stage.assert_same(got, refs[r][j], outs[r])
    return dev, jobs, from_dev


def check_relaunch_and_short_workspace(stage, dev, from_dev, packed, outs, jobs, same_again):
    """The last part of the same test: a second launch on the same buffers gives the same answer (the call initialises everything
    it reads), and a workspace one byte too small is WT_ERR_CAPACITY with nothing launched.  Returns the refused device form."""
    import torch
    from waymo_2d_tracking_amd import _lib
    dev.launch()
    again = dev.results()
    assert len(again) == len(from_dev), stage.name
    for k, (a, b) in enumerate(zip(from_dev, again)):
        assert same_again(a, b), (stage.name, 'job %d differs after a second launch' % k)
    small = stage.device(packed, outs, jobs, workspace_bytes=dev.ws_bytes - 1)
    with pytest.raises(_lib.WaymoTrackError, match='WT_ERR_CAPACITY'):
        small.launch()
    torch.cuda.synchronize()
    return small


def check_shuffled(stage, packed, out, jobs, refs, per_row):
    """The unsorted / shuffled input test: the rows in a random order give what the reference gives for that order, and
    per_row(got, the reference of the sorted input, the permutation) holds - the stage's own statement about every row."""
    perm = np.random.default_rng(4).permutation(len(out['frame']))
    shuffled = dict((k, v[perm]) for k, v in out.items())
    got = stage.tracks(packed, [shuffled], jobs)
    assert len(got) == len(jobs) == len(refs), (stage.name, len(got))
    for g, j, ref in zip(got, jobs, refs):
        stage.assert_same(g, stage.reference(packed['stream_frame_offsets'], shuffled, j), shuffled)
        per_row(g, ref, perm)


def check_cli_default_flags(golden_dir, tmp_path, extras, module=None):
    """test_cli_default_flags_write_what_they_wrote: with the stage's flags absent or at their defaults (`extras`: flag lists),
    on both io paths, track.py writes the tracker's own rows - and does not even import `module`."""
    from waymo_2d_tracking_amd.tracking import track, utils as T
    kept = sys.modules.get(module)
    try:
        for fixture, score in (('sort_g5_input.json', '0.95,0.6,1.0,0.9'), ('sort_g4_input.json', '0.3,0.3,1.0,0.2')):
            path = os.path.join(golden_dir, fixture)
            flags = ['--input', path, '--max-age=2', '--score-threshold=' + score]
            T.reset_global_ids(0)
            untouched = json.dumps(T.track_all(T.read_data_file(path, [float(v) for v in score.split(',')]), [0.01, 0.01, 1.0, 0.0], 2, 0))
            sys.modules.pop(module, None)                                  # the tests before this one imported it
            written = []
            for i, extra in enumerate([[], ['--python-io']] + list(extras)):
                T.reset_global_ids(0)
                assert track.main(flags + ['--output', str(tmp_path / ('t%d.json' % i))] + extra) == 0, (fixture, extra)
                written.append((tmp_path / ('t%d.json' % i)).read_text())
            assert written[1] == untouched, (fixture, '--python-io')
            for i, w in enumerate(written):
                assert w == written[1], (fixture, 'run %d' % i)
            assert module is None or module not in sys.modules, (fixture, module)
        exp = json.load(open(os.path.join(golden_dir, 'sort_g4_expected_a.json')))['tracks']
        ids = lambda rows: [(r['image_id'], r['category_id'], r['object_id']) for r in rows]
        assert ids(json.loads(written[0])) == ids(exp), 'sort_g4_expected_a.json'
    finally:
        if kept is not None:
            sys.modules[module] = kept
