"""Cross-class track linking restated in plain Python: per-trajectory lists, Python floats and ints, the
candidate pairs as one sorted list walked once.  Built differently from csrc/track_xlink.hip on purpose - the kernel never holds
the list of pairs, matches in rounds of mutually best pairs and votes by walking a chain once per class; here every pair is
listed, sorted and walked once, and a chain's rows are counted in a dict.

Definition.  Trajectories, their local index by first appearance, a trajectory's class (the category of its first observation),
iou_dd and extrapolate / predicted_box are those of tests/stitch_ref.py.  A job = {'pairs': {(a, b): {'max_link': G, 'link_iou': T}},
'prio': one int or one per class (default 0), 'motion': 'hold' | 'linear'}: unordered pairs of classes 1..n_classes (at most 16),
(a, a) allowed, a pair that is not named is off, one given twice is an error.
  1. Candidates: tail i of class ci (last observation at slot e) and head j != i of the same stream and class cj (first observation
     at slot s), n = s - e, 1 <= n <= max_link[ci][cj], affinity a >= link_iou[ci][cj] and a > 0.  The affinity is stitching's rule 2.
  2. Matching: walk the candidates in the strict order (-a, n, i, j); accept when i is not yet a tail and j not yet a head.
  3. Vote: a chain = a root and everything linked behind it; its class is the c that maximises (rows of the chain's pieces whose
     class is c, prio[c - 1], 1 if c is the root's class else 0, -c) among the classes with at least one row.
  4. Output: every row takes the root's object_id and the chain's class; per trajectory pred, root, affinity, cls; per row the
     root's local index and the category; per stream the links and the rows whose category changed."""
import stitch_ref
from stitch_ref import MOTIONS, match_greedy, match_mutual_best, order_key, trajectories

MAX_CLASSES = 16


def tables(pairs, n_classes):
    """({(ci, cj): max_link}, {(ci, cj): link_iou}) over ordered class pairs; a pair that is absent is off"""
    if n_classes > MAX_CLASSES:
        raise ValueError('at most %d classes' % MAX_CLASSES)
    gap, thr, seen = {}, {}, set()
    for (a, b), v in pairs.items():
        a, b = int(a), int(b)
        if not (1 <= a <= n_classes and 1 <= b <= n_classes):
            raise ValueError('pair (%d, %d): classes are 1..%d' % (a, b, n_classes))
        if frozenset((a, b)) in seen:
            raise ValueError('pair (%d, %d) is given twice (pairs are unordered)' % (a, b))
        seen.add(frozenset((a, b)))
        g, t = int(v.get('max_link', 1)), float(v.get('link_iou', 0.3))
        if g < 0 or t != t:
            raise ValueError('max_link must be >= 0 and link_iou must not be NaN')
        gap[(a, b)] = gap[(b, a)] = g
        thr[(a, b)] = thr[(b, a)] = t
    return gap, thr


def prio_of(job, n_classes):
    prio = job.get('prio', 0)
    prio = [int(v) for v in prio] if isinstance(prio, (list, tuple)) else [int(prio)]
    if len(prio) == 1:
        prio = prio * n_classes
    if len(prio) != n_classes:
        raise ValueError('prio need one value, or one per class (%d)' % n_classes)
    return prio


def candidates(trajs, job, n_classes):
    """the candidate pairs of one stream: (a, n, i, j), unordered"""
    gap, thr = tables(job.get('pairs', {}), n_classes)
    found = []
    for i, (_, ci, tail) in enumerate(trajs):
        for j, (_, cj, head) in enumerate(trajs):
            if i == j or gap.get((ci, cj), 0) < 1:
                continue
            n = head[0][0] - tail[-1][0]
            if n < 1 or n > gap[(ci, cj)]:
                continue
            a = stitch_ref.affinity([(o[0], o[1]) for o in tail], [(o[0], o[1]) for o in head], job.get('motion', 'hold'))
            if a >= thr[(ci, cj)] and a > 0.0:
                found.append((a, n, i, j))
    return found


def vote(members, trajs, root, prio):
    """the class of the chain `members` (local indices) with root `root`"""
    rows = {}
    for t in members:
        rows[trajs[t][1]] = rows.get(trajs[t][1], 0) + len(trajs[t][2])
    return max(rows, key=lambda c: (rows[c], prio[c - 1], 1 if c == trajs[root][1] else 0, -c))


def xlink(stream_frame_offsets, out, job, n_classes=4, key=order_key):
    """out: dict of sequences frame, category, bbox, object_id (score is not read).  Returns a dict: object_id, category and
    row_root per row in the caller's order; pred, root, affinity, cls per trajectory, stream after stream in local index order,
    with traj_offsets (one entry per stream + 1); n_links, n_relabelled per stream; links = (from id, to id, gap, affinity) per
    accepted link, stream after stream, ascending head index."""
    if job.get('motion', 'hold') not in MOTIONS:
        raise ValueError("motion must be 'hold' or 'linear'")
    prio = prio_of(job, n_classes)
    n_streams = len(stream_frame_offsets) - 1
    per_stream = trajectories(stream_frame_offsets, out)
    n = len(out['frame'])
    result = {'object_id': [int(v) for v in out['object_id']], 'category': [int(v) for v in out['category']], 'row_root': [-1] * n,
              'pred': [], 'root': [], 'affinity': [], 'cls': [], 'traj_offsets': [0], 'n_links': [], 'n_relabelled': [], 'links': []}
    for s in range(n_streams):
        trajs = per_stream.get(s, [])
        links = match_greedy(candidates(trajs, job, n_classes), key)
        roots, chains = [], {}
        for j in range(len(trajs)):
            root = j
            while root in links:
                root = links[root][0]
            roots.append(root)
            chains.setdefault(root, []).append(j)
        cls = dict((root, vote(members, trajs, root, prio)) for root, members in chains.items())
        relabelled = 0
        for j in range(len(trajs)):
            root = roots[j]
            result['pred'].append(links[j][0] if j in links else -1)
            result['affinity'].append(links[j][1] if j in links else -1.0)
            result['root'].append(root)
            result['cls'].append(cls[root])
            for _, _, row in trajs[j][2]:
                result['object_id'][row] = trajs[root][0]
                result['row_root'][row] = root
                relabelled += result['category'][row] != cls[root]
                result['category'][row] = cls[root]
            if j in links:
                result['links'].append((trajs[links[j][0]][0], trajs[j][0], links[j][2], links[j][1]))
        result['n_links'].append(len(links))
        result['n_relabelled'].append(relabelled)
        result['traj_offsets'].append(len(result['pred']))
    return result
