"""Track refinement restated in plain Python: per-trajectory lists, Python floats, one operation per
statement.  Built differently from csrc/track_refine.hip on purpose - no tables, no scans, no links between rows: every
trajectory is collected as a list, filtered and filled on its own, and the output is sorted at the end.

Definition.  A tracking result = the rows utils.track_packed returns (frame = index of the frame slot, category, bbox
[x1, y1, w, h], score, object_id).  Slots belong to streams (stream_frame_offsets).  A trajectory = the rows of one stream with the
same object_id, ordered by slot; its class is the category of its first observation and selects max_gap[class - 1] and
min_len[class - 1].
  1. A trajectory with fewer than min_len observations is removed (counted before any filling).
  2. Between consecutive observations a at slot fa and b at slot fb, n = fb - fa, 2 <= n <= max_gap + 1: one row at each slot
     fa + j, j = 1 .. n - 1, with each of x1, y1, w, h, score = va + (vb - va) * (j / n), every operation rounded on its own;
     it copies category and object_id of a.
  3. score_mode 'mean': every row of the trajectory carries ((s0 + s1) + s2 ...) / count over its observed scores in slot order.
  4. Order: slot; inside a slot the surviving observed rows in input order, then the filled rows in ascending trajectory index,
     trajectories numbered by first appearance in the stream.
  5. source: input row index for an observed row, -1 - (input row index of b) for a filled one.
Rows that are not sorted by frame are sorted stably first; source keeps the caller's indices."""


def stream_of_slot(stream_frame_offsets, slot):
    for s in range(len(stream_frame_offsets) - 1):
        if stream_frame_offsets[s] <= slot < stream_frame_offsets[s + 1]:
            return s
    raise ValueError('slot %d is in no stream' % slot)


def interpolate(va, vb, j, n):
    t = float(j) / float(n)
    d = vb - va
    m = d * t
    return va + m


def mean_in_order(scores):
    total = scores[0]
    for s in scores[1:]:
        total = total + s
    return total / float(len(scores))


def refine(stream_frame_offsets, out, job):
    """out: dict of sequences frame, category, bbox, score, object_id; job: {'max_gap': [per class], 'min_len': [per class],
    'score_mode': 'keep' | 'mean'}.  Returns a dict of lists: frame, category, bbox, score, object_id, source, and
    frame_row_offsets (one entry per slot + 1)."""
    offsets = [int(v) for v in stream_frame_offsets]
    n_slots = offsets[-1]
    n = len(out['frame'])
    rows = [(int(out['frame'][i]), int(out['category'][i]), [float(v) for v in out['bbox'][i]], float(out['score'][i]),
             int(out['object_id'][i]), i) for i in range(n)]
    rows_sorted = sorted(rows, key=lambda r: r[0])                    # stable: input order inside a slot
    position = {}
    for pos, r in enumerate(rows_sorted):
        position[r[5]] = pos
    # trajectories, per stream, in order of first appearance
    trajectories = {}
    for r in rows_sorted:
        s = stream_of_slot(offsets, r[0])
        per_stream = trajectories.setdefault(s, {})
        per_stream.setdefault(r[4], []).append(r)
    emitted = []                                                      # (slot, 0 observed / 1 filled, order inside, row)
    for s in sorted(trajectories):
        for index, (oid, obs) in enumerate(trajectories[s].items()):
            slots = [r[0] for r in obs]
            if len(set(slots)) != len(slots):
                raise ValueError('object_id %d occurs twice in slot %d' % (oid, [f for f in slots if slots.count(f) > 1][0]))
            c = obs[0][1]
            max_gap = int(job['max_gap'][c - 1])
            min_len = int(job['min_len'][c - 1])
            if len(obs) < min_len:
                continue
            mean = mean_in_order([r[3] for r in obs]) if job['score_mode'] == 'mean' else None
            for r in obs:
                score = mean if mean is not None else r[3]
                emitted.append((r[0], 0, position[r[5]], (r[0], r[1], list(r[2]), score, oid, r[5])))
            for a, b in zip(obs[:-1], obs[1:]):
                gap = b[0] - a[0]
                if gap < 2 or gap > max_gap + 1:
                    continue
                for j in range(1, gap):
                    box = [interpolate(a[2][i], b[2][i], j, gap) for i in range(4)]
                    score = mean if mean is not None else interpolate(a[3], b[3], j, gap)
                    emitted.append((a[0] + j, 1, index, (a[0] + j, a[1], box, score, oid, -1 - b[5])))
    emitted.sort(key=lambda e: e[:3])
    result = {'frame': [], 'category': [], 'bbox': [], 'score': [], 'object_id': [], 'source': []}
    for e in emitted:
        for name, v in zip(('frame', 'category', 'bbox', 'score', 'object_id', 'source'), e[3]):
            result[name].append(v)
    result['frame_row_offsets'] = [sum(1 for f in result['frame'] if f < slot) for slot in range(n_slots + 1)]
    return result
