"""TEST INFRASTRUCTURE - deterministic stand-ins for everything tracking/evaluate.py's sweep() and main() run on the device, and
the characterization cases that pin their host logic (tests/test_sweep_host.py, oracle/gen_golden_sweep.py).

sweep() reaches the tracker (utils.track_packed, utils.track_packed_byte), the five post-passes (split / stitch / dedup / refine /
smooth `*_tracks`) and the four evaluators (evaluate.evaluate_*) through module attributes at call time; `installed()` replaces
them all, so the enumeration of the settings, the per-class pick, the ranking, the flag line and the printed and written documents
run on a machine without a GPU.

A fake result has one row whose box encodes what was done to it: the tracker's box is a CRC of its arguments, a stage's box a CRC
of (input box, stage name, the job's parameters without 'result') - a job whose switch value is off hands the input box on, so that
default second-axis values tie exactly.  The evaluators build real result objects from counts drawn from a generator seeded with
the CRC of the row's box.  Every fake appends (name, len(outs), len(jobs), crc of its arguments) to LOG."""
import contextlib
import hashlib
import io
import json
import os
import zlib

import numpy as np

from waymo_2d_tracking_amd import synthetic
from waymo_2d_tracking_amd.tracking import evaluate as E
from waymo_2d_tracking_amd.tracking import utils as T

LOG = []
PIN_LIMIT = 20000                                   # longer texts are pinned by their SHA-256 (the fixture stays small)
N_GT, N_HYP, N_TRAJ = 12, 11, 5                     # constant over the settings, as on real data: tp can exceed neither


def _plain(v):
    if isinstance(v, (list, tuple, np.ndarray)):
        return [_plain(x) for x in v]
    if isinstance(v, (bool, str)) or v is None:
        return v
    if isinstance(v, (int, np.integer)):
        return int(v)
    return float(v)


def crc(*parts):
    return zlib.crc32(repr(_plain(parts)).encode())


def _row(code):
    return dict(frame=np.zeros(1, np.int64), category=np.ones(1, np.int32), bbox=np.asarray([[code & 0xffff, code >> 16, 10, 10]], np.float64),
                score=np.ones(1, np.float64), object_id=np.ones(1, np.int64))


def _code(out):
    return int(out['bbox'][0, 0]) | int(out['bbox'][0, 1]) << 16


def track_packed(packed, iou_thresholds, max_age, min_hits, score_threshold=None, id_base=0):
    code = crc('track_packed', iou_thresholds, max_age, min_hits, score_threshold, id_base)
    LOG.append(('track_packed', 0, 1, code))
    return _row(code), 1


def track_packed_byte(packed, iou_thresholds, max_age, min_hits, score_threshold, low_score_threshold, low_iou_thresholds, id_base=0):
    code = crc('track_packed_byte', iou_thresholds, max_age, min_hits, score_threshold, low_score_threshold, low_iou_thresholds, id_base)
    LOG.append(('track_packed_byte', 0, 1, code))
    return _row(code), 1


def _stage(name, off):
    def run(packed, outs, jobs, n_classes=4):
        LOG.append((name, len(outs), len(jobs), crc([_code(o) for o in outs], [sorted(j.items()) for j in jobs], n_classes)))
        results = []
        for job in jobs:
            code = _code(outs[job.get('result', 0)])
            if not off(job):
                code = crc(code, name, sorted((k, v) for k, v in job.items() if k != 'result'))
            results.append(_row(code))
        return results
    run.__name__ = name
    return run


STAGES = {'split': _stage('split_tracks', lambda j: j['split_iou'] == 0 and j['split_gap'] == 0),
          'stitch': _stage('stitch_tracks', lambda j: j['max_link'] == 0),
          'dedup': _stage('dedup_tracks', lambda j: j['min_frames'] == 0),
          'refine': _stage('refine_tracks', lambda j: j['max_gap'] == 0 and j['min_len'] == 1),
          'smooth': _stage('smooth_tracks', lambda j: j['window'] == 0)}


def _draws(tr):
    """(seed, generator of non-negative ints) for one result: a 64-bit LCG seeded with the CRC of the first row's x and y."""
    seed = crc(int(tr['x'][0]), int(tr['y'][0])) if tr['x'].size else 0

    def gen(state=seed):
        while True:
            state = (state * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
            yield state >> 33
    return seed, gen()


def _cells(gt, tr, n_classes):
    """(stream, class index, level index, draws) of every cell of one result; every fourth result has nothing of class 2 at all."""
    seed, d = _draws(tr)
    for s in range(len(gt['stream_keys'])):
        for c in range(n_classes):
            for li in range(2):
                if not (c == 1 and seed % 4 == 0):
                    yield s, c, li, d


def _logged(name, tracks_list, iou_threshold, packed):
    LOG.append((name, len(tracks_list), 0, crc([[tr['x'], tr['y']] for tr in tracks_list], iou_threshold, packed is not None)))


def evaluate_tracks(gt, tracks_list, iou_threshold=E.DEFAULT_IOU_THRESHOLD, per_row=False, packed=None):
    _logged('evaluate_tracks', tracks_list, iou_threshold, packed)
    results = []
    for tr in tracks_list:
        counts = np.zeros((len(gt['stream_keys']), len(iou_threshold), 2, 5), np.int64)
        iou_sum = np.zeros(counts.shape[:3], np.float64)
        for s, c, li, d in _cells(gt, tr, len(iou_threshold)):
            tp = next(d) % (N_HYP + 1)
            counts[s, c, li] = (N_GT, tp, N_GT - tp, N_HYP - tp, next(d) % 3)
            iou_sum[s, c, li] = tp * (0.5 + (next(d) % 1000) / 2000)
        results.append(E.MotResult(counts, iou_sum, 0, gt['stream_keys']))
    return results


def evaluate_identity(gt, tracks_list, iou_threshold=E.DEFAULT_IOU_THRESHOLD, per_row=False, workspace_limit_bytes=None, packed=None):
    _logged('evaluate_identity', tracks_list, iou_threshold, packed)
    results = []
    for tr in tracks_list:
        counts = np.zeros((len(gt['stream_keys']), len(iou_threshold), 2, 3), np.int64)
        for s, c, li, d in _cells(gt, tr, len(iou_threshold)):
            counts[s, c, li] = (next(d) % (N_HYP + 1), N_GT, N_HYP)
        results.append(E.IdentityResult(counts, 0, gt['stream_keys']))
    return results


def evaluate_hota(gt, tracks_list, iou_threshold=E.DEFAULT_IOU_THRESHOLD, per_row=False, workspace_limit_bytes=None, packed=None):
    _logged('evaluate_hota', tracks_list, iou_threshold, packed)
    results = []
    for tr in tracks_list:
        counts = np.zeros((len(gt['stream_keys']), len(iou_threshold), 2, 2 + E.N_ALPHAS), np.int64)
        sums = np.zeros(counts.shape[:3] + (E.N_ALPHAS, 4), np.float64)
        for s, c, li, d in _cells(gt, tr, len(iou_threshold)):
            tp = [next(d) % (N_HYP + 1) for _ in range(E.N_ALPHAS)]
            counts[s, c, li] = [N_GT, N_HYP] + tp
            sums[s, c, li] = [[t * (next(d) % 1000) / 1000 for _ in range(4)] for t in tp]
        results.append(E.HotaResult(counts, sums, 0, gt['stream_keys']))
    return results


def evaluate_coverage(gt, tracks_list, iou_threshold=E.DEFAULT_IOU_THRESHOLD, per_trajectory=False, packed=None):
    _logged('evaluate_coverage', tracks_list, iou_threshold, packed)
    results = []
    for tr in tracks_list:
        counts = np.zeros((len(gt['stream_keys']), len(iou_threshold), 2, 5), np.int64)
        for s, c, li, d in _cells(gt, tr, len(iou_threshold)):
            mt = next(d) % (N_TRAJ + 1)
            pt = next(d) % (N_TRAJ + 1 - mt)
            counts[s, c, li] = (N_TRAJ, mt, pt, N_TRAJ - mt - pt, next(d) % 4)
        results.append(E.CoverageResult(counts, 0, gt['stream_keys']))
    return results


@contextlib.contextmanager
def installed():
    """Everything the sweep runs on the device replaced by the fakes, LOG emptied; the real attributes come back on exit."""
    from waymo_2d_tracking_amd.tracking import dedup, refine, smooth, split, stitch
    targets = [(T, 'track_packed', track_packed), (T, 'track_packed_byte', track_packed_byte)]
    targets += [(module, name + '_tracks', STAGES[name]) for module, name in
                ((split, 'split'), (stitch, 'stitch'), (dedup, 'dedup'), (refine, 'refine'), (smooth, 'smooth'))]
    targets += [(E, f.__name__, f) for f in (evaluate_tracks, evaluate_identity, evaluate_hota, evaluate_coverage)]
    saved = [(module, name, getattr(module, name)) for module, name, _ in targets]
    del LOG[:]
    for module, name, fake in targets:
        setattr(module, name, fake)
    try:
        yield LOG
    finally:
        for module, name, real in saved:
            setattr(module, name, real)


# ---------------------------------------------------------------------------------------------------------------
# the characterization cases
BASE = {'score': [0.3, 0.6], 'iou': [0.01, 0.1], 'max_age': [1, 2], 'min_hits': [0, 1]}
ONE = {'score': [0.3], 'iou': [0.01], 'max_age': [1], 'min_hits': [0]}
DEFAULTS = {'gap': [0], 'min_len': [1], 'link_gap': [0], 'link_iou': [0.3], 'link_motion': 'hold', 'split_iou': [0.0], 'split_gap': 0,
            'split_motion': 'linear', 'dedup_frames': [0], 'dedup_iou': [0.7], 'dedup_frac': 0.5, 'smooth_window': [0], 'smooth_sigma': [1.0],
            'smooth_kernel': 'gaussian', 'low_score': [], 'low_iou': [0.5]}
SINGLE_PASS = {'split': {'split_iou': [0.0, 0.4], 'split_gap': 2, 'split_motion': 'hold'},
               'stitch': {'link_gap': [0, 3], 'link_iou': [0.3, 0.6], 'link_motion': 'linear'},
               'dedup': {'dedup_frames': [0, 3], 'dedup_iou': [0.5, 0.7], 'dedup_frac': 0.25},
               'refine': {'gap': [0, 2], 'min_len': [1, 3]},
               'smooth': {'smooth_window': [0, 2], 'smooth_sigma': [1.0, 2.0], 'smooth_kernel': 'box'},
               'second': {'low_score': [0.2, 0.5], 'low_iou': [0.3, 0.5]}}
EVERYTHING = {'score': [0.3, 0.6], 'iou': [0.01], 'max_age': [1, 2], 'min_hits': [0], 'low_score': [0.2, 0.5], 'low_iou': [0.5],
              'split_iou': [0.0, 0.4], 'split_gap': 2, 'split_motion': 'hold', 'link_gap': [0, 3], 'link_iou': [0.3], 'link_motion': 'linear',
              'dedup_frames': [0, 3], 'dedup_iou': [0.7], 'dedup_frac': 0.25, 'gap': [0, 2], 'min_len': [1],
              'smooth_window': [0, 2], 'smooth_sigma': [1.0], 'smooth_kernel': 'box'}
EVERYTHING_FLAGS = ['--score-grid', '0.3,0.6', '--iou-grid', '0.01', '--max-age', '1,2', '--min-hits', '0', '--low-score-grid', '0.2,0.5',
                    '--low-iou-grid', '0.5', '--split-iou-grid', '0,0.4', '--split-gap', '2', '--split-motion', 'hold', '--link-gap-grid', '0,3',
                    '--link-iou-grid', '0.3', '--link-motion', 'linear', '--dedup-frames-grid', '0,3', '--dedup-iou-grid', '0.7',
                    '--dedup-frac', '0.25', '--gap-grid', '0,2', '--min-len-grid', '1', '--smooth-window-grid', '0,2',
                    '--smooth-sigma-grid', '1.0', '--smooth-kernel', 'box']


def text(value):
    return json.dumps(value, sort_keys=True)


def pin(value):
    """What the fixture holds for one recorded item: its JSON text, or the text's SHA-256 and length where it is long."""
    t = value if isinstance(value, str) else text(value)
    return t if len(t) <= PIN_LIMIT else {'sha256': hashlib.sha256(t.encode()).hexdigest(), 'chars': len(t)}


def write_inputs(directory):
    """det.json, gt.json and two tracking files in `directory`; returns the detections and the ground truth."""
    dets, gt_json = synthetic.make_tracking_json(23, n_segments=1, n_frames=4, n_objects=4, cameras=('FRONT', 'SIDE_LEFT'))
    rows = [dict(image_id=d['image_id'], bbox=d['bbox'], category_id=d['category_id'], object_id=i % 3) for i, d in enumerate(dets)]
    # tracks_b.json begins with a row that makes it one of the results without class 2: its tables show the NaN scores
    b = next(i for i in range(6, len(rows)) if crc(int(rows[i]['bbox'][0]), int(rows[i]['bbox'][1])) % 4 == 0)
    for name, doc in (('det.json', dets), ('gt.json', gt_json), ('tracks_a.json', rows[:6]), ('tracks_b.json', rows[b:b + 5])):
        with open(os.path.join(directory, name), 'wt') as fp:
            json.dump(doc, fp)
    return dets, gt_json


def sweep_record(name, grid, **kw):
    """One sweep under the fakes -> {item name: pinned text}."""
    with installed() as log:
        res = E.sweep('det.json', 'gt.json', grid, **kw)
        log = [list(entry) for entry in log]
    return {name + '/settings': pin(res['settings']), name + '/ranked': pin(res['ranked']), name + '/best': pin(res['best']),
            name + '/flag_lines': pin(dict((lv, [E.flag_line(r) for r in rows]) for lv, rows in res['ranked'].items())),
            name + '/log': pin(log)}


def main_record(name, argv, out_path):
    """One run of evaluate.main under the fakes -> its standard output, its --json document key by key, and the call log."""
    stdout = io.StringIO()
    with installed() as log, contextlib.redirect_stdout(stdout):
        assert E.main(argv + ['--json', out_path]) == 0
        log = [list(entry) for entry in log]
    with open(out_path) as fp:
        doc = json.load(fp)
    items = {name + '/stdout': pin(stdout.getvalue()), name + '/json_keys': pin(list(doc)), name + '/log': pin(log)}
    for key, value in doc.items():
        if isinstance(value, dict) and name == 'main_tables':
            for sub, v in value.items():
                items['%s/json/%s/%s' % (name, key, sub)] = pin(v)
        else:
            items['%s/json/%s' % (name, key)] = pin(value)
    return items


def everything_sweep(rank_by):
    return sweep_record('everything_by_' + rank_by, EVERYTHING, identity=True, hota=True, coverage=True, rank_by=rank_by)


def run_cases(directory):
    """Every characterization case, run in `directory` (the inputs are written there) -> {item name: pinned text}."""
    cwd = os.getcwd()
    os.chdir(directory)
    try:
        write_inputs('.')
        items = {}
        items.update(sweep_record('base', BASE))
        items.update(sweep_record('base_with_defaults', dict(BASE, **DEFAULTS)))
        for name, axes in SINGLE_PASS.items():
            items.update(sweep_record('only_' + name, dict(ONE, **axes), identity=True, hota=True, coverage=True))
        for rank_by in ('mota', 'idf1', 'hota', 'mt'):
            items.update(everything_sweep(rank_by))
        gt = E.load_ground_truth('gt.json')
        one = [E.load_tracks('tracks_b.json')]
        for kind, evaluate, fmt in (('mot', evaluate_tracks, E.format_table), ('identity', evaluate_identity, E.format_identity_table),
                                    ('hota', evaluate_hota, E.format_hota_table), ('coverage', evaluate_coverage, E.format_coverage_table)):
            result = evaluate(gt, one, E.DEFAULT_IOU_THRESHOLD)[0]
            items['result_%s/table' % kind] = pin(fmt(result, 'tracks_b.json'))
            items['result_%s/as_json' % kind] = pin(result.as_json())
        items.update(main_record('main_sweep', ['--annotations', 'gt.json', '--sweep', 'det.json'] + EVERYTHING_FLAGS +
                                 ['--rank-by', 'hota', '--identity', '--coverage'], 'sweep_out.json'))
        items.update(main_record('main_tables', ['--annotations', 'gt.json', 'tracks_a.json', 'tracks_b.json', '--identity', '--hota', '--coverage'],
                                 'tables_out.json'))
        return items
    finally:
        os.chdir(cwd)
