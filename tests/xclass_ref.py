"""Cross-class track suppression restated in plain Python: per-trajectory lists, Python floats and ints, one
operation per statement, every pair of trajectories looked at, one sorted walk.  Built differently from csrc/track_xclass.hip on
purpose - the kernel never holds the pairs and decides in rounds; here the trajectories are sorted by strength and walked once.

Definition.  Results, slots, streams, trajectories, local indices by first appearance, a trajectory's class c_t (the category of
its first observation), n_t and s_t are those of the deduplication (tests/dedup_ref.py).  A job = frames[a][b] >= 0 (0 = the pair
of classes a + 1, b + 1 is off), overlap[a][b] (not NaN), frac[a][b] in 0..1 - three symmetric C x C tables - prio[c] and measure
('iou' or 'iomin').  A trajectory whose class is outside 1..C takes part in no pair.
  1. Measure of two boxes, with w, h, wh, area_a, area_b as iou_dd computes them: IoU = iou_dd; IoMin = wh / lo, lo the smaller
     area, only when area_a > 0, area_b > 0 and both are finite - otherwise nothing.  A slot matches when v >= overlap and v > 0.
  2. Strength: t before u by higher prio[c], then more rows, then higher score sum, then lower local index.
  3. Same object: frames[c_t][c_u] > 0, m(t, u) >= frames[c_t][c_u], float(m) >= frac[c_t][c_u] * float(n_weak), n_weak the rows
     of the WEAKER of the two.
  4. Walk from strongest to weakest: suppressed when a stronger KEPT trajectory is the same object; by = the strongest such one,
     match = m with it; kept: by = -1, match = 0.  All rows of a suppressed trajectory go; nothing else changes."""
import math
import struct

import dedup_ref

MEASURES = ('iou', 'iomin')


def bits(v):
    return struct.pack('<d', v)


def tables(job, n_classes):
    """(frames, overlap, frac, prio, measure) of a job: lists of lists.  A job names unordered 'pairs' {(a, b): {'frames',
    'overlap', 'frac'}}, or carries the three tables themselves; the tables must be symmetric, the floats bit for bit."""
    C = n_classes
    if 'pairs' in job or 'frames' not in job:
        frames = [[0] * C for _ in range(C)]
        overlap = [[0.7] * C for _ in range(C)]
        frac = [[0.5] * C for _ in range(C)]
        for (a, b), v in job.get('pairs', {}).items():
            for i, k in ((a - 1, b - 1), (b - 1, a - 1)):
                frames[i][k] = int(v.get('frames', 3))
                overlap[i][k] = float(v.get('overlap', 0.7))
                frac[i][k] = float(v.get('frac', 0.5))
    else:
        frames, overlap, frac = job['frames'], job['overlap'], job['frac']
    prio = job.get('prio', 0)
    prio = [int(v) for v in prio] if isinstance(prio, (list, tuple)) else [int(prio)] * C
    measure = job.get('measure', 'iomin')
    if measure not in MEASURES:
        raise ValueError('measure %r' % (measure,))
    for a in range(C):
        for b in range(C):
            if frames[a][b] < 0:
                raise ValueError('frames of pair (%d, %d) is negative' % (a + 1, b + 1))
            if overlap[a][b] != overlap[a][b]:
                raise ValueError('overlap of pair (%d, %d) is NaN' % (a + 1, b + 1))
            if not 0.0 <= frac[a][b] <= 1.0:
                raise ValueError('frac of pair (%d, %d) is outside 0..1' % (a + 1, b + 1))
            if frames[a][b] != frames[b][a] or bits(overlap[a][b]) != bits(overlap[b][a]) or bits(frac[a][b]) != bits(frac[b][a]):
                raise ValueError('pair (%d, %d) and pair (%d, %d) differ' % (a + 1, b + 1, b + 1, a + 1))
    return frames, overlap, frac, prio, measure


def iomin_dd(a, b):
    """intersection over the smaller area of two boxes [x1, y1, x2, y2], from the terms of csrc/eval_device.h iou_dd; NaN = nothing"""
    xx1 = a[0] if a[0] > b[0] else b[0]
    yy1 = a[1] if a[1] > b[1] else b[1]
    xx2 = a[2] if a[2] < b[2] else b[2]
    yy2 = a[3] if a[3] < b[3] else b[3]
    w = xx2 - xx1
    if not w > 0.0:
        w = 0.0
    h = yy2 - yy1
    if not h > 0.0:
        h = 0.0
    wh = w * h
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[2] - b[0]) * (b[3] - b[1])
    if not (area_a > 0.0 and area_b > 0.0 and area_a < math.inf and area_b < math.inf):
        return float('nan')
    lo = area_a if area_a < area_b else area_b
    return wh / lo


def naive_iomin(a, b):
    """the OTHER measure, without the guard: wh over min(area) - the cases use it to show what the guard keeps out"""
    w = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    h = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    lo = min((a[2] - a[0]) * (a[3] - a[1]), (b[2] - b[0]) * (b[3] - b[1]))
    return w * h / lo if lo != 0.0 else float('nan')


def measure_of(name, a, b):
    return dedup_ref.iou_dd(a, b) if name == 'iou' else iomin_dd(a, b)


def match_count(t, u, thr, measure):
    m = 0
    for slot in sorted(t.obs):
        if slot not in u.obs:
            continue
        v = measure_of(measure, dedup_ref.corners(t.obs[slot][0]), dedup_ref.corners(u.obs[slot][0]))
        if v >= thr and v > 0.0:
            m += 1
    return m


def strength_key(trajs, prio, t):
    c = trajs[t].category
    p = prio[c - 1] if 1 <= c <= len(prio) else 0
    return (-p, -trajs[t].n, -trajs[t].score_sum, t)


def stronger(trajs, prio, t, u):
    return strength_key(trajs, prio, t) < strength_key(trajs, prio, u)


def strength_order(trajs, prio):
    return sorted(range(len(trajs)), key=lambda t: strength_key(trajs, prio, t))


def same_objects(trajs, job, n_classes):
    """{(t, u): m} for t < u, the pairs of one stream that are the same object"""
    frames, overlap, frac, prio, measure = tables(job, n_classes)
    found = {}
    for t in range(len(trajs)):
        for u in range(t + 1, len(trajs)):
            ct, cu = trajs[t].category, trajs[u].category
            if not (1 <= ct <= n_classes and 1 <= cu <= n_classes):
                continue
            if not frames[ct - 1][cu - 1] > 0:
                continue
            m = match_count(trajs[t], trajs[u], overlap[ct - 1][cu - 1], measure)
            weak = u if stronger(trajs, prio, t, u) else t
            need = frac[ct - 1][cu - 1] * float(trajs[weak].n)
            if m >= frames[ct - 1][cu - 1] and float(m) >= need:
                found[(t, u)] = m
    return found


def suppress_greedy(trajs, pairs, prio, suppressed_suppress=False):
    """rule 4: (keep, by, match) per trajectory.  suppressed_suppress: the OTHER rule, where a stronger match suppresses whether it
    was kept or not."""
    T = len(trajs)
    m_of = lambda t, u: pairs.get((t, u) if t < u else (u, t))
    keep, by, match = [1] * T, [-1] * T, [0] * T
    walked = []
    for t in strength_order(trajs, prio):
        for s in walked:                              # strongest first
            if m_of(s, t) is not None and (keep[s] or suppressed_suppress):
                keep[t], by[t], match[t] = 0, s, m_of(s, t)
                break
        walked.append(t)
    return keep, by, match


def suppress_in_rounds(trajs, pairs, prio):
    """The same answer the way the kernel reaches it: every round, each undecided trajectory with no undecided stronger match is
    decided.  Returns (keep, by, match, rounds)."""
    T = len(trajs)
    state = [0] * T                                   # 0 undecided, 1 kept, 2 suppressed
    by, match, rounds = [-1] * T, [0] * T, 0
    ordered = [(t, u) if stronger(trajs, prio, t, u) else (u, t) for t, u in pairs]
    while 0 in state:
        rounds += 1
        pending, proposal = set(), {}
        for s, w in ordered:
            if state[w] != 0:
                continue
            if state[s] == 0:
                pending.add(w)
            elif state[s] == 1 and (w not in proposal or stronger(trajs, prio, s, proposal[w])):
                proposal[w] = s
        decided = [t for t in range(T) if state[t] == 0 and t not in pending]
        assert decided                                # the strongest undecided one is never pending
        for t in decided:
            state[t] = 2 if t in proposal else 1
            if t in proposal:
                s = proposal[t]
                by[t], match[t] = s, pairs[(t, s) if t < s else (s, t)]
    return [1 if v == 1 else 0 for v in state], by, match, rounds


def xclass(stream_frame_offsets, out, job, n_classes=4, suppressed_suppress=False):
    """out: dict of sequences frame, category, bbox, score, object_id; job: as tracking/xclass.py takes it.  Returns a dict of lists
    of the form dedup_ref.dedup returns: keep, by, match per trajectory with traj_offsets, n_dropped per stream, dropped = (object
    id, suppressor's object id, m), row_keep per input row in the caller's order, and the surviving rows."""
    n_streams = len(stream_frame_offsets) - 1
    prio = tables(job, n_classes)[3]
    per_stream = dedup_ref.trajectories(stream_frame_offsets, out)
    n = len(out['frame'])
    result = {'keep': [], 'by': [], 'match': [], 'row_keep': [1] * n, 'n_dropped': [], 'traj_offsets': [0], 'dropped': []}
    for s in range(n_streams):
        trajs = per_stream.get(s, [])
        keep, by, match = suppress_greedy(trajs, same_objects(trajs, job, n_classes), prio, suppressed_suppress)
        for t in range(len(trajs)):
            if keep[t]:
                continue
            for slot in trajs[t].obs:
                result['row_keep'][trajs[t].obs[slot][1]] = 0
            result['dropped'].append((trajs[t].object_id, trajs[by[t]].object_id, match[t]))
        result['keep'] += keep
        result['by'] += by
        result['match'] += match
        result['n_dropped'].append(len(keep) - sum(keep))
        result['traj_offsets'].append(len(result['keep']))
    rows = [i for i in range(n) if result['row_keep'][i]]
    result['frame'] = [int(out['frame'][i]) for i in rows]
    result['category'] = [int(out['category'][i]) for i in rows]
    result['bbox'] = [[float(v) for v in out['bbox'][i]] for i in rows]
    result['score'] = [float(out['score'][i]) for i in rows]
    result['object_id'] = [int(out['object_id'][i]) for i in rows]
    return result


def from_dedup_job(job, n_classes=4):
    """the job of this pass that a deduplication job (tests/dedup_cases.job) reduces to: diagonal pairs only, equal priorities, IoU"""
    pairs = dict(((c, c), {'frames': int(job['min_frames'][c - 1]), 'overlap': float(job['dup_iou'][c - 1]), 'frac': float(job['dup_frac'][c - 1])})
                 for c in range(1, n_classes + 1))
    return {'pairs': pairs, 'prio': [0] * n_classes, 'measure': 'iou'}
