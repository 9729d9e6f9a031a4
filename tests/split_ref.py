"""Track splitting restated in plain Python: per-trajectory lists, Python floats, one operation per
statement.  Built differently from csrc/track_split.hip on purpose - the kernel links rows, decides every pair in a lane of its own
and counts with scans; here a trajectory is a list that is walked once.

Definition.  A tracking result = the rows utils.track_packed returns.  A trajectory = the rows of one stream with the same
object_id, ordered by slot; trajectories of a stream are numbered by first appearance (the local index); a trajectory's class is the
category of its first observation.  A job = split_iou[class - 1] (not NaN; <= 0: the IoU rule is off), split_gap[class - 1] >= 0
(0: the gap rule is off), motion 'hold' | 'linear'.
Observations of a trajectory at slots f_0 < ... < f_{m-1}; the pair (i - 1, i), n = f_i - f_{i-1}:
  1. Gap rule: the pair breaks when split_gap > 0 and n > split_gap.
  2. IoU rule (split_iou > 0); the tests that exist:
       forward  (linear, i >= 2):     p = f_{i-1} - f_{i-2}; px = x_{i-1} + ((x_{i-1} - x_{i-2}) / p) * n, py alike; w, h of row i - 1;
                                      a_f = iou([px, py, px + w, py + h], box_i)
       backward (linear, i + 1 < m):  q = f_{i+1} - f_i; px = x_i + ((x_i - x_{i+1}) / q) * n, py alike; w, h of row i;
                                      a_b = iou(pred, box_{i-1})
       hold     (neither exists):     a_h = iou(box_{i-1}, box_i)
     The pair breaks when every existing test gives a < split_iou; a NaN never breaks.  Every operation rounded on its own.
  3. piece(row) = the breaking pairs of its trajectory at or before the row.  Piece 0 keeps the identity; the other pieces of a
     result are numbered from 0 in the order (stream, local index, piece): new(row), -1 for piece 0.  Such a row gets the id
     first_new_id + new(row).
Rows that are not sorted by frame are sorted stably first; the per-row outputs stay in the caller's order."""
from stitch_ref import iou_dd, trajectories

MOTIONS = ('hold', 'linear')


def extrapolate(v, v_other, slots, n):
    """v + ((v - v_other) / slots) * n, one operation per statement"""
    step = v - v_other
    rate = step / float(slots)
    move = rate * float(n)
    return v + move


def corners(box):
    x, y, w, h = box
    return [x, y, x + w, y + h]


def pair_tests(obs, i, motion):
    """obs: the trajectory's observations (slot, box) in slot order; the tests of the pair (i - 1, i), i >= 1, as (a_f or a_h or
    None, a_b or None)"""
    n = obs[i][0] - obs[i - 1][0]
    first, second = None, None
    if motion == 'linear' and i >= 2:
        p = obs[i - 1][0] - obs[i - 2][0]
        x, y, w, h = obs[i - 1][1]
        px = extrapolate(x, obs[i - 2][1][0], p, n)
        py = extrapolate(y, obs[i - 2][1][1], p, n)
        first = iou_dd([px, py, px + w, py + h], corners(obs[i][1]))
    if motion == 'linear' and i + 1 < len(obs):
        q = obs[i + 1][0] - obs[i][0]
        x, y, w, h = obs[i][1]
        px = extrapolate(x, obs[i + 1][1][0], q, n)
        py = extrapolate(y, obs[i + 1][1][1], q, n)
        second = iou_dd([px, py, px + w, py + h], corners(obs[i - 1][1]))
    if first is None and second is None:
        first = iou_dd(corners(obs[i - 1][1]), corners(obs[i][1]))
    return first, second


def pair_breaks(n, tests, split_iou, split_gap):
    if split_gap > 0 and n > split_gap:
        return True
    if not split_iou > 0.0:
        return False
    existing = [a for a in tests if a is not None]
    return all(a < split_iou for a in existing)


def split(stream_frame_offsets, out, job):
    """out: dict of sequences frame, category, bbox, object_id (score is not read); job: {'split_iou': [per class], 'split_gap':
    [per class], 'motion': 'hold' | 'linear', 'first_new_id': int, default the largest object id + 1}.  Returns a dict: object_id,
    piece, new and test ([a_f or a_h or -1.0, a_b or -1.0]) per row in the caller's order; breaks per trajectory, stream after
    stream in local index order, with traj_offsets (one entry per stream + 1); n_new_pieces per stream and their sum n_new."""
    assert job['motion'] in MOTIONS
    n_streams = len(stream_frame_offsets) - 1
    n_rows = len(out['frame'])
    ids = [int(v) for v in out['object_id']]
    first_new_id = job.get('first_new_id')
    if first_new_id is None:
        first_new_id = max(ids) + 1 if ids else 0
    per_stream = trajectories(stream_frame_offsets, out)
    result = {'object_id': ids, 'piece': [-1] * n_rows, 'new': [-1] * n_rows, 'test': [[-1.0, -1.0] for _ in range(n_rows)],
              'breaks': [], 'traj_offsets': [0], 'n_new_pieces': [], 'n_new': 0}
    made = 0
    for s in range(n_streams):
        before = made
        for _, cls, rows in per_stream.get(s, []):
            split_iou = float(job['split_iou'][cls - 1])
            split_gap = int(job['split_gap'][cls - 1])
            obs = [(slot, box) for slot, box, _ in rows]
            piece = 0
            for i, (_, _, row) in enumerate(rows):
                if i >= 1:
                    tests = (None, None)
                    if split_iou > 0.0:
                        tests = pair_tests(obs, i, job['motion'])
                        result['test'][row] = [-1.0 if a is None else a for a in tests]
                    if pair_breaks(obs[i][0] - obs[i - 1][0], tests, split_iou, split_gap):
                        piece += 1
                result['piece'][row] = piece
                if piece > 0:
                    result['new'][row] = made + piece - 1
                    result['object_id'][row] = first_new_id + made + piece - 1
            result['breaks'].append(piece)
            made += piece
        result['n_new_pieces'].append(made - before)
        result['traj_offsets'].append(len(result['breaks']))
    result['n_new'] = made
    return result
