"""What the case modules of the track post-passes (tests/*_cases.py, DESIGN.md sections 20-26) share: the form of a hand-made result."""

N_CLASSES = 4


def result(rows):
    """rows: (slot, category, [x, y, w, h], score, object_id)"""
    return {'frame': [r[0] for r in rows], 'category': [r[1] for r in rows], 'bbox': [list(r[2]) for r in rows],
            'score': [r[3] for r in rows], 'object_id': [r[4] for r in rows]}


def by_slot(rows):
    return sorted(rows, key=lambda r: r[0])           # stable: the order of first appearance is the order given
