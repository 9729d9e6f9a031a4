"""Host composition of the file route for K views' wire slots (helpers of tests/test_gpu_view_ensemble.py).

Every view's slots are read as the columns of one exported detection file (one image per frame, rows in slot order), then
merged by the same steps as `python -m waymo_2d_tracking_amd.detnet.ensemble`: merge_inputs -> pack_groups -> the CPU
oracle's ensemble_groups -> score > min_score, boxes truncated, numpy's round(score, 5).  The result is laid out like
wt_ensemble_slots_dev's output: per frame K * S slots, groups in ascending category order, then empty slots."""
import numpy as np

from waymo_2d_tracking_amd.detnet import ensemble as E


def slots_as_submission(xywhs, category, n_frames, slots):
    """One view's slots (5, F * S), (F * S) -> read_submission-style columns (image = frame index, slot order kept)."""
    idx = np.nonzero(category != 0)[0]
    return dict(image=(idx // slots).astype(np.int32), category=category[idx].astype(np.int32),
                x=xywhs[0, idx].astype(np.float64), y=xywhs[1, idx].astype(np.float64),
                w=xywhs[2, idx].astype(np.float64), h=xywhs[3, idx].astype(np.float64),
                score=xywhs[4, idx].astype(np.float64), image_ids=list(range(n_frames)))


def host_merge_slots(oracle, xywhs, category, n_frames, slots, weights, method, iou_thresh, soft_nms_cut, min_score):
    """xywhs (K, 5, F * S), category (K, F * S) -> (out_xywhs (5, F * K * S), out_category (F * K * S), counts (F))."""
    K = len(weights)
    subs = [slots_as_submission(xywhs[k], category[k], n_frames, slots) for k in range(K)]
    image_ids, category_ids, rows = E.merge_inputs(subs, weights, min_score)
    out_x = np.zeros((5, n_frames * K * slots))
    out_c = np.zeros(n_frames * K * slots, np.int32)
    counts = np.zeros(n_frames, np.int64)
    if not image_ids:
        return out_x, out_c, counts
    packed = E.pack_groups(len(image_ids), category_ids, rows, K)
    out5, cnt = oracle.ensemble_groups(packed['dets5'], packed['group_offsets'], packed['input_sizes'], K,
                                       E.METHODS[method], iou_thresh, soft_nms_cut)
    ncat = packed['ncat']
    for g in range(packed['n_groups']):
        frame = int(image_ids[g // ncat])
        o = int(packed['group_offsets'][g])
        r = out5[o:o + int(cnt[g])]
        r = r[r[:, 0] > min_score]
        a = frame * K * slots + int(counts[frame])
        out_x[0:4, a:a + len(r)] = np.trunc(r[:, 1:5]).T
        out_x[4, a:a + len(r)] = np.round(r[:, 0], 5)
        out_c[a:a + len(r)] = category_ids[g % ncat]
        counts[frame] += len(r)
    return out_x, out_c, counts


def random_view_slots(rng, K, n_frames, slots, n_categories):
    """Wire slots of K views of the same frames: integer boxes, 5-decimal scores; empty slots, zero-width rows, scores
    below a typical min_score, exact cross-view duplicates and exact score ties included."""
    N = n_frames * slots
    xywhs = np.zeros((K, 5, N))
    cat = np.zeros((K, N), np.int32)
    for f in range(n_frames):
        n_obj = int(rng.integers(0, slots // 2))
        base = np.stack([rng.integers(0, 1800, n_obj), rng.integers(0, 1200, n_obj), rng.integers(4, 300, n_obj),
                         rng.integers(4, 200, n_obj)], axis=0).astype(np.float64)
        bscore = np.round(rng.uniform(0.0, 1.0, n_obj), 5)
        bcat = rng.integers(1, n_categories + 1, n_obj).astype(np.int32)
        for k in range(K):
            n = int(rng.integers(0, slots + 1))
            pick = rng.integers(0, max(n_obj, 1), n) if n_obj else np.zeros(0, np.int64)
            n = len(pick)
            b = base[:, pick] + rng.integers(-6, 7, (4, n))
            exact = rng.random(n) < 0.25                              # exact copies of the base box (cross-view duplicates)
            b[:, exact] = base[:, pick[exact]]
            s = np.where(rng.random(n) < 0.3, bscore[pick], np.round(np.clip(bscore[pick] + rng.normal(0, 0.05, n), 0, 1), 5))
            s[rng.random(n) < 0.1] = 0.005                            # below min_score
            b[2, rng.random(n) < 0.05] = 0.0                          # zero width
            b[3, rng.random(n) < 0.03] = -1.0                         # negative height
            c = bcat[pick].copy()
            c[rng.random(n) < 0.1] = 0                                # empty slot in the middle
            sl = f * slots + np.sort(rng.choice(slots, n, replace=False))
            xywhs[k, 0:4, sl] = b.T
            xywhs[k, 4, sl] = s
            cat[k, sl] = c
    return xywhs, cat
