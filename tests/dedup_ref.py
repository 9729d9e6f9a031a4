"""Track deduplication restated in plain Python: per-trajectory lists, Python floats and ints, one operation
per statement, every pair of trajectories looked at, one sorted walk.  Built differently from csrc/track_dedup.hip on purpose - the
kernel never holds the pairs and decides in rounds; here the trajectories are sorted by strength and walked once.

Definition.  A tracking result = the rows utils.track_packed returns.  A trajectory = the rows of one stream with the same
object_id, ordered by slot; trajectories of a stream are numbered by first appearance (the local index); a trajectory's class is the
category of its first observation.  A job = min_frames[class - 1] >= 0, dup_iou[class - 1] (not NaN), dup_frac[class - 1] in 0..1.
  1. Per trajectory t: n_t rows, class c_t, score sum s_t = 0.0 + score + score + ... in slot order.
  2. Strength: t before u when n_t > n_u, or equal and s_t > s_u, or both equal and t < u.  Scores must be finite.
  3. m(t, u) = the slots where both have a row and a = iou(box_t, box_u) has a >= dup_iou[c] and a > 0.
  4. Duplicates: c_t == c_u == c, min_frames[c] > 0, m >= min_frames[c], float(m) >= dup_frac[c] * float(min(n_t, n_u)).
  5. Walk from strongest to weakest: suppressed when a stronger KEPT trajectory is a duplicate; by = the strongest such one,
     match = m with it; kept: by = -1, match = 0.  All rows of a suppressed trajectory go; nothing else changes.
Rows that are not sorted by frame are sorted stably first; the per-row outputs stay in the caller's order."""
import math


def stream_of_slot(stream_frame_offsets, slot):
    for s in range(len(stream_frame_offsets) - 1):
        if stream_frame_offsets[s] <= slot < stream_frame_offsets[s + 1]:
            return s
    raise ValueError('slot %d is in no stream' % slot)


def iou_dd(a, b):
    """csrc/eval_device.h iou_dd: two boxes [x1, y1, x2, y2], every operation on its own"""
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
    total = area_a + area_b
    union = total - wh
    if union == 0.0:                                  # C division: 0 / 0 is NaN, v / 0 is an infinity
        return float('nan') if wh == 0.0 or wh != wh else float('inf')
    return wh / union


def corners(box):
    x, y, w, h = box
    return [x, y, x + w, y + h]


class Trajectory(object):
    def __init__(self, object_id, category):
        self.object_id, self.category = object_id, category
        self.obs = {}                                 # slot -> (box, caller's row)
        self.n, self.score_sum = 0, 0.0

    def add(self, slot, box, score, row):
        if slot in self.obs:
            raise ValueError('object_id %d occurs twice in slot %d' % (self.object_id, slot))
        if not math.isfinite(score):
            raise ValueError('row %d: score is not finite' % row)
        self.obs[slot] = (box, row)
        self.n = self.n + 1
        self.score_sum = self.score_sum + score


def trajectories(stream_frame_offsets, out):
    """{stream: [Trajectory]} in order of first appearance"""
    offsets = [int(v) for v in stream_frame_offsets]
    rows = [(int(out['frame'][i]), int(out['category'][i]), [float(v) for v in out['bbox'][i]], float(out['score'][i]), int(out['object_id'][i]), i)
            for i in range(len(out['frame']))]
    per_stream = {}
    for slot, cat, box, score, oid, i in sorted(rows, key=lambda r: r[0]):        # stable: input order inside a slot
        trajs = per_stream.setdefault(stream_of_slot(offsets, slot), {})
        if oid not in trajs:
            trajs[oid] = Trajectory(oid, cat)
        trajs[oid].add(slot, box, score, i)
    return dict((s, list(t.values())) for s, t in per_stream.items())


def match_count(t, u, thr):
    m = 0
    for slot in sorted(t.obs):
        if slot not in u.obs:
            continue
        a = iou_dd(corners(t.obs[slot][0]), corners(u.obs[slot][0]))
        if a >= thr and a > 0.0:
            m += 1
    return m


def stronger(trajs, t, u):
    a, b = trajs[t], trajs[u]
    if a.n != b.n:
        return a.n > b.n
    if a.score_sum != b.score_sum:
        return a.score_sum > b.score_sum
    return t < u


def strength_order(trajs):
    return sorted(range(len(trajs)), key=lambda t: (-trajs[t].n, -trajs[t].score_sum, t))


def duplicates(trajs, job):
    """{(t, u): m} for t < u, the duplicate pairs of one stream"""
    found = {}
    for t in range(len(trajs)):
        for u in range(t + 1, len(trajs)):
            c = trajs[t].category
            if c != trajs[u].category:
                continue
            min_frames = int(job['min_frames'][c - 1])
            if not min_frames > 0:
                continue
            m = match_count(trajs[t], trajs[u], float(job['dup_iou'][c - 1]))
            shorter = trajs[t].n if trajs[t].n < trajs[u].n else trajs[u].n
            need = float(job['dup_frac'][c - 1]) * float(shorter)
            if m >= min_frames and float(m) >= need:
                found[(t, u)] = m
    return found


def suppress_greedy(trajs, dups, suppressed_suppress=False):
    """rule 5: (keep, by, match) per trajectory.  suppressed_suppress: the OTHER rule, where a stronger duplicate suppresses
    whether it was kept or not - the cases use it to show that the two rules differ."""
    T = len(trajs)
    m_of = lambda t, u: dups.get((t, u) if t < u else (u, t))
    keep, by, match = [1] * T, [-1] * T, [0] * T
    walked = []
    for t in strength_order(trajs):
        for s in walked:                              # strongest first
            if m_of(s, t) is not None and (keep[s] or suppressed_suppress):
                keep[t], by[t], match[t] = 0, s, m_of(s, t)
                break
        walked.append(t)
    return keep, by, match


def suppress_in_rounds(trajs, dups):
    """The same answer the way the kernel reaches it: every round, each undecided trajectory with no undecided stronger
    duplicate is decided.  Returns (keep, by, match, rounds)."""
    T = len(trajs)
    state = [0] * T                                   # 0 undecided, 1 kept, 2 suppressed
    by, match, rounds = [-1] * T, [0] * T, 0
    pairs = [(t, u) if stronger(trajs, t, u) else (u, t) for t, u in dups]
    while 0 in state:
        rounds += 1
        pending, proposal = set(), {}
        for s, w in pairs:
            if state[w] != 0:
                continue
            if state[s] == 0:
                pending.add(w)
            elif state[s] == 1 and (w not in proposal or stronger(trajs, s, proposal[w])):
                proposal[w] = s
        decided = [t for t in range(T) if state[t] == 0 and t not in pending]
        assert decided                                # the strongest undecided one is never pending
        for t in decided:
            state[t] = 2 if t in proposal else 1
            if t in proposal:
                s = proposal[t]
                by[t], match[t] = s, dups[(t, s) if t < s else (s, t)]
    return [1 if v == 1 else 0 for v in state], by, match, rounds


def dedup(stream_frame_offsets, out, job, suppressed_suppress=False):
    """out: dict of sequences frame, category, bbox, score, object_id; job: {'min_frames': [per class], 'dup_iou': [per class],
    'dup_frac': [per class]}.  Returns a dict of lists: keep, by, match per trajectory, stream after stream in local index order,
    with traj_offsets (one entry per stream + 1); n_dropped per stream; dropped = (object id, suppressor's object id, m) per
    suppressed trajectory in that order; row_keep per input row in the caller's order; and the surviving rows' frame, category,
    bbox, score and object_id in the caller's order."""
    n_streams = len(stream_frame_offsets) - 1
    per_stream = trajectories(stream_frame_offsets, out)
    n = len(out['frame'])
    result = {'keep': [], 'by': [], 'match': [], 'row_keep': [1] * n, 'n_dropped': [], 'traj_offsets': [0], 'dropped': []}
    for s in range(n_streams):
        trajs = per_stream.get(s, [])
        keep, by, match = suppress_greedy(trajs, duplicates(trajs, job), suppressed_suppress)
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
