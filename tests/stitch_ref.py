"""Track stitching restated in plain Python: per-trajectory lists, Python floats, one operation per
statement, the candidate pairs as one sorted list.  Built differently from csrc/track_stitch.hip on purpose - the kernel never
holds the list of pairs and matches in rounds of mutually best pairs; here every pair is listed, sorted and walked once.

Definition.  A tracking result = the rows utils.track_packed returns.  A trajectory = the rows of one stream with the same
object_id, ordered by slot; trajectories of a stream are numbered by first appearance (the local index); a trajectory's class is the
category of its first observation.  A job = max_link[class - 1] >= 0, link_iou[class - 1] (not NaN), motion 'hold' | 'linear'.
  1. Candidates: tail i (last observation at slot e, box x, y, w, h, the observation before it at slot p) and head j != i of the
     same stream and class (first observation at slot s), n = s - e, 1 <= n <= max_link, affinity a >= link_iou and a > 0.
  2. Affinity: linear with two observations: px = x + ((x - x_p) / (e - p)) * n, py alike; otherwise px = x, py = y; every
     operation rounded on its own.  a = iou([px, py, px + w, py + h], [xh, yh, xh + wh, yh + hh]) in the order of iou_dd.
  3. Matching: walk the candidates in the strict order (-a, n, i, j); accept when i is not yet a tail and j not yet a head.
  4. Output: every row takes the object_id of its chain's root; per trajectory pred, root, affinity; per row the root's local
     index; per stream the links.
Rows that are not sorted by frame are sorted stably first; the per-row outputs stay in the caller's order."""

MOTIONS = ('hold', 'linear')


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


def extrapolate(v, v_before, e, p, n):
    step = v - v_before
    rate = step / float(e - p)
    move = rate * float(n)
    return v + move


def predicted_box(obs, n, motion):
    """obs: the tail's observations (slot, box) in slot order; the box n slots after its last one, [x1, y1, x2, y2]"""
    e, (x, y, w, h) = obs[-1]
    px, py = x, y
    if motion == 'linear' and len(obs) >= 2:
        p, before = obs[-2]
        px = extrapolate(x, before[0], e, p, n)
        py = extrapolate(y, before[1], e, p, n)
    return [px, py, px + w, py + h]


def affinity(tail_obs, head_obs, motion):
    n = head_obs[0][0] - tail_obs[-1][0]
    x, y, w, h = head_obs[0][1]
    return iou_dd(predicted_box(tail_obs, n, motion), [x, y, x + w, y + h])


def trajectories(stream_frame_offsets, out):
    """{stream: [(object_id, class, [(slot, box, caller's row)])]} in order of first appearance"""
    offsets = [int(v) for v in stream_frame_offsets]
    rows = [(int(out['frame'][i]), int(out['category'][i]), [float(v) for v in out['bbox'][i]], int(out['object_id'][i]), i)
            for i in range(len(out['frame']))]
    per_stream = {}
    for r in sorted(rows, key=lambda r: r[0]):        # stable: input order inside a slot
        per_stream.setdefault(stream_of_slot(offsets, r[0]), {}).setdefault(r[3], []).append(r)
    result = {}
    for s, trajs in per_stream.items():
        result[s] = []
        for oid, obs in trajs.items():
            slots = [r[0] for r in obs]
            if len(set(slots)) != len(slots):
                raise ValueError('object_id %d occurs twice in slot %d' % (oid, [f for f in slots if slots.count(f) > 1][0]))
            result[s].append((oid, obs[0][1], [(r[0], r[2], r[4]) for r in obs]))
    return result


def candidates(trajs, job):
    """the candidate pairs of one stream: (a, n, i, j), unordered"""
    found = []
    for i, (_, ci, tail) in enumerate(trajs):
        for j, (_, cj, head) in enumerate(trajs):
            if i == j or ci != cj:
                continue
            n = head[0][0] - tail[-1][0]
            if n < 1 or n > int(job['max_link'][ci - 1]):
                continue
            a = affinity([(o[0], o[1]) for o in tail], [(o[0], o[1]) for o in head], job['motion'])
            if a >= float(job['link_iou'][ci - 1]) and a > 0.0:
                found.append((a, n, i, j))
    return found


def order_key(c):
    return (-c[0], c[1], c[2], c[3])


def match_greedy(cands, key=order_key):
    """rule 3: {head: (tail, a, n)}"""
    tails, links = set(), {}
    for a, n, i, j in sorted(cands, key=key):
        if i in tails or j in links:
            continue
        tails.add(i)
        links[j] = (i, a, n)
    return links


def match_mutual_best(cands, key=order_key):
    """Rounds of locally dominant pairs: every free pair that is its tail's best free candidate and its head's best free candidate
    is accepted together.  Returns ({head: (tail, a, n)}, rounds that accepted something)."""
    tails, links, rounds = set(), {}, 0
    while True:
        free = [c for c in cands if c[2] not in tails and c[3] not in links]
        if not free:
            return links, rounds
        best_of_tail, best_of_head = {}, {}
        for c in free:
            if c[2] not in best_of_tail or key(c) < key(best_of_tail[c[2]]):
                best_of_tail[c[2]] = c
            if c[3] not in best_of_head or key(c) < key(best_of_head[c[3]]):
                best_of_head[c[3]] = c
        accepted = [c for c in best_of_tail.values() if best_of_head[c[3]] is c]
        assert accepted                               # the smallest free pair is always one
        for a, n, i, j in accepted:
            tails.add(i)
            links[j] = (i, a, n)
        rounds += 1


def stitch(stream_frame_offsets, out, job, key=order_key):
    """out: dict of sequences frame, category, bbox, object_id (score is not read); job: {'max_link': [per class],
    'link_iou': [per class], 'motion': 'hold' | 'linear'}.  Returns a dict: object_id and row_root per row in the caller's order;
    pred, root, affinity per trajectory, stream after stream in local index order, with traj_offsets (one entry per stream + 1);
    n_links per stream; links = (from id, to id, gap, affinity) per accepted link, stream after stream, ascending head index."""
    assert job['motion'] in MOTIONS
    n_streams = len(stream_frame_offsets) - 1
    per_stream = trajectories(stream_frame_offsets, out)
    result = {'object_id': [int(v) for v in out['object_id']], 'row_root': [-1] * len(out['frame']), 'pred': [], 'root': [],
              'affinity': [], 'traj_offsets': [0], 'n_links': [], 'links': []}
    for s in range(n_streams):
        trajs = per_stream.get(s, [])
        links = match_greedy(candidates(trajs, job), key)
        for j in range(len(trajs)):
            root = j
            while root in links:
                root = links[root][0]
            result['pred'].append(links[j][0] if j in links else -1)
            result['affinity'].append(links[j][1] if j in links else -1.0)
            result['root'].append(root)
            for _, _, row in trajs[j][2]:
                result['object_id'][row] = trajs[root][0]
                result['row_root'][row] = root
            if j in links:
                result['links'].append((trajs[links[j][0]][0], trajs[j][0], links[j][2], links[j][1]))
        result['n_links'].append(len(links))
        result['traj_offsets'].append(len(result['pred']))
    return result
