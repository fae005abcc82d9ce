"""
Shapes and input sets of the K2a forward tests, shared by tests/test_collision_model.py (CPU: is every set what it claims to be, judged on the
model alone?) and tests/test_gpu_collision_paths.py (GPU: do the kernels agree with the oracle and the model on them?).

Dispatch of tds_collision_f32 (csrc/collision.hip), for the `path` column:
    scene = collision_scene_iou_kernel   metric iou, A * N <= 4096 and (4 * 1024 + 6 * N + 2 * A * N) * 4 bytes of LDS <= 65536
    row   = collision_kernel<METRIC>     everything else: all of discs, and iou scenes that are too large for the scene kernel
"""
import numpy as np

# (A, N), metrics, path for iou (discs always takes the row kernel), why
SHAPES = [
    ((1, 1), ('iou', 'discs'), 'scene'),        # sum - max = 0, partner -1
    ((8, 11), ('iou', 'discs'), 'scene'),       # the shape of the goldens with NPCs
    ((64, 64), ('iou', 'discs'), 'scene'),      # A * N = 4096 exactly; bit 63
    ((8, 512), ('iou',), 'scene'),              # 8 chunks of 64 partners; 61 440 B of LDS
    ((6, 682), ('iou',), 'scene'),              # 65 488 of 65 536 B; N % 64 = 42
    ((5, 819), ('iou',), 'row'),                # A * N = 4095 <= 4096, but 68 800 B of LDS: falls to the row kernel
    ((64, 65), ('iou', 'discs'), 'row'),        # the first scene over 4096 pairs; a last chunk of one lane
    ((17, 129), ('iou', 'discs'), 'scene'),     # discs: 16 rows per block, so the second block holds one row; iou: 2193 pairs, 37 KB -> scene
    ((17, 257), ('iou',), 'row'),               # the same for the iou row kernel: 4369 pairs; a last chunk of one lane
    ((4, 1024), ('iou', 'discs'), 'row'),       # the example of the launcher's comment (73.7 KB for the scene kernel)
    ((2, 3136), ('iou', 'discs'), 'row'),       # the first N past 3072
    ((1, 8192), ('iou', 'discs'), 'row'),       # the documented maximum of N
]
SETS = ('mixed', 'ties', 'scrub', 'rim')        # rim: iou only (it is about the cull of the Rotated-IoU pipeline)

ORIGINS = (0.0, 400.0, 3000.0)                  # cluster origins in metres: fp32 spacing of the coordinates grows 1 : 64 : 512 over them
PITCH, COLUMNS = 16.0, 20                       # lay-out grid: boxes are at most 12 m long and jittered by 1 m, so grid neighbours never touch


def expected_path(A, N, metric):
    lds_scene = (4 * 16 * 64 + 6 * N + 2 * A * N) * 4
    return 'scene' if metric == 'iou' and A * N <= 4096 and lds_scene <= 64 * 1024 else 'row'


def batch_of(N):
    return 2 if N >= 1024 else 3


def cases():
    """(A, N, metric, set) of every test case"""
    out = []
    for (A, N), metrics, path in SHAPES:
        for metric in metrics:
            assert expected_path(A, N, metric) == (path if metric == 'iou' else 'row')
            for s in SETS:
                if s == 'rim' and metric != 'iou':
                    continue
                out.append((A, N, metric, s))
    return out


def _grid(gen, B, N):
    """collision-free lay-out: box k of a scene sits in cluster k % 3, on a 16 m grid of 20 columns, jittered by up to 1 m"""
    k = np.arange(N)
    cl, slot = k % 3, k // 3
    x = np.asarray(ORIGINS)[cl] + PITCH * (slot % COLUMNS)
    y = PITCH * (slot // COLUMNS)
    xy = np.stack([x, y], -1)[None] + gen.uniform(-1.0, 1.0, (B, N, 2))
    length, width = gen.uniform(3.5, 12.0, (B, N)), gen.uniform(1.6, 2.6, (B, N))
    wide = gen.uniform(size=(B, N)) < 0.12                        # width > length: the angle switch of the discs metric
    length, width = np.where(wide, width, length), np.where(wide, length, width)
    psi = gen.uniform(-np.pi, np.pi, (B, N))
    return np.concatenate([xy, length[..., None], width[..., None], psi[..., None]], -1)


def _near(gen, box, spread=1.6):
    """a copy of `box`'s position moved by up to `spread` metres per axis: overlaps it for every size drawn above (all are >= 1.6 m wide)"""
    return box[:2] + gen.uniform(-spread, spread, 2)


def _mixed(gen, B, A, N, frac=0.5):
    boxes = _grid(gen, B, N)
    present = gen.uniform(size=(B, N)) >= 0.15
    if A <= 2:
        present[:, :A] = True                                        # too few rows to lose one
    if N == 1:
        return boxes, present
    for b in range(B):
        # about half of the rows get one to three boxes moved onto them, taken from the top of the index range (so that partners lie in the
        # last chunk, and bit 63 is used when N = 64); where most boxes are rows the moved ones are rows themselves, so fewer are chosen
        rows = gen.permutation(A)[:max(1, int(round(A * frac * (0.4 if N - A < A else 1.0))))]
        if A == 1:
            rows = rows[:1] if b % 2 == 0 else rows[:0]               # one row per scene: every other scene collides
        top = N - 1
        for n, i in enumerate(rows):
            for v in range(1 + n % 3):
                while top in rows or top == i:
                    top -= 1
                if top < 0:
                    break
                boxes[b, top, :2] = _near(gen, boxes[b, i], 0.6 if v == 0 else 1.6)
                top -= 1
    return boxes, present


def _ties(gen, B, A, N):
    """Box 3 and box N - 1 are copies of box `src` = 1 (of box 0 when that is the only row), a long box laid out below the grid, and so is box 1:
    small rows placed along it without touching each other see one and the same overlap three times, within the first chunk and across the
    chunks -- and row `src` itself sees its copies at its own self overlap, which is larger than the small rows' overlaps with it."""
    boxes, present = _mixed(gen, B, A, N, frac=0.3)
    if N < 7:
        return boxes, present
    src = 1 if A >= 2 else 0
    for b in range(B):
        psi = gen.uniform(-np.pi, np.pi)
        along = np.array([np.cos(psi), np.sin(psi)])
        boxes[b, src] = (ORIGINS[b % 3] + gen.uniform(5.0, 9.0), -40.0 + gen.uniform(-1.0, 1.0), 12.0, 2.4, psi)
        for k, i in enumerate((0, 2, 4, 5)):
            if i < A and i != src:                                   # 3.2 m apart along the long box: further than their diagonal of 3.17 m
                boxes[b, i, :2] = boxes[b, src, :2] + (3.2 * k - 4.8) * along + gen.uniform(-0.3, 0.3, 2)
                boxes[b, i, 2:4] = (2.6, 1.8)
        if A >= 7:
            boxes[b, N - 2, :2] = _near(gen, boxes[b, 6], 0.5)       # and one row whose only partner lies in the last chunk
            present[b, [6, N - 2]] = True
        boxes[b, 1] = boxes[b, src]
        boxes[b, 3] = boxes[b, src]
        boxes[b, N - 1] = boxes[b, src]
        present[b, [0, 1, 2, 3, N - 1]] = True
    return boxes, present


def _scrub(gen, B, A, N):
    boxes, present = _mixed(gen, B, A, N)
    if N < 7:
        if N > 1:
            boxes[0, N - 1, 4] = np.nan
        boxes[-1, 0, 0] = np.nan
        return boxes, present
    for b in range(B):
        # rows 0 .. 2 (as far as they exist) each get an NPC with one NaN field on top of them; the row is placed where the scrubbed NPC lands
        j_x, j_psi, j_len, j_abs = N - 1, N - 2, N - 3, N - 4
        i0, i1, i2 = 0, min(1, A - 1), min(2, A - 1)
        boxes[b, i0, 0] = 0.7                                        # NaN x scrubs to x = 0
        boxes[b, j_x, :2] = (np.nan, boxes[b, i0, 1] + 0.6)
        boxes[b, j_psi, :2] = _near(gen, boxes[b, i1], 1.0)
        boxes[b, j_psi, 2:4] = (2.0, 9.0) if b % 2 == 0 else (9.0, 2.0)   # a NaN heading on a box wider than long, and on a long one
        boxes[b, j_psi, 4] = np.nan
        boxes[b, j_len, :2] = _near(gen, boxes[b, i2], 0.8)
        boxes[b, j_len, 2] = np.nan                                  # length 0 after the scrub: a degenerate rectangle inside row i2's box
        present[b, [j_x, j_psi, j_len, j_abs]] = True
        if b == 0:
            boxes[b, 0, 4] = np.nan                                  # and a NaN heading on a row itself
        # one absent exposed agent under two present boxes: its self overlap is masked, the maximum is one of the others
        ia = A - 1 if A - 1 < N - 5 else 3
        present[b, ia] = False
        boxes[b, j_abs, :2] = _near(gen, boxes[b, ia], 1.0)
        if N - 5 > 3 and N - 5 != ia:
            boxes[b, N - 5, :2] = _near(gen, boxes[b, ia], 1.0)
            present[b, N - 5] = True
    return boxes, present


def reach_f32(b1, b2):
    """the bounding-circle test of iou_pair (csrc/collision.hip) restated in float32: (d2, reach2), culled iff d2 > reach2"""
    f = np.float32
    b1, b2 = b1.astype(f), b2.astype(f)
    dx, dy = b1[..., 0] - b2[..., 0], b1[..., 1] - b2[..., 1]
    r1 = f(0.5) * np.sqrt(b1[..., 2] * b1[..., 2] + b1[..., 3] * b1[..., 3])
    r2 = f(0.5) * np.sqrt(b2[..., 2] * b2[..., 2] + b2[..., 3] * b2[..., 3])
    big = np.maximum(np.maximum(np.abs(b1[..., 0]), np.abs(b1[..., 1])), np.maximum(np.abs(b2[..., 0]), np.abs(b2[..., 1])))
    reach = r1 + r2 + f(0.05) + f(1e-5) * big
    return dx * dx + dy * dy, reach * reach


def _rim(gen, B, A, N):
    """pairs whose centre distance is within 2 mm of the cull threshold r1 + r2 + 0.05 + 1e-5 * max|coord|: rows are chained along x within
    their cluster, and the NPCs are dealt round-robin onto circles of that radius around the rows"""
    boxes = _grid(gen, B, N)
    boxes[..., 1] += 40.0                                            # keep max|coord| away from 0 so that the 1e-5 term is live everywhere
    present = gen.uniform(size=(B, N)) >= 0.1

    side = [1.0]

    def place(b, j, i, theta):
        c = boxes[b, i]
        for _ in range(3):                                           # the threshold depends on where j lands: fixed-point iteration
            r1 = 0.5 * np.hypot(c[2], c[3])
            r2 = 0.5 * np.hypot(boxes[b, j, 2], boxes[b, j, 3])
            big = max(abs(c[0]), abs(c[1]), abs(boxes[b, j, 0]), abs(boxes[b, j, 1]))
            d = r1 + r2 + 0.05 + 1e-5 * big
            boxes[b, j, :2] = c[:2] + d * np.array([np.cos(theta), np.sin(theta)])
        side[0] = -side[0]                                           # alternately just inside and just outside
        d += side[0] * gen.uniform(1e-4, 2e-3)
        boxes[b, j, :2] = c[:2] + d * np.array([np.cos(theta), np.sin(theta)])

    for b in range(B):
        # row i hangs on row i - 3, the previous row of its cluster; a small scene is one chain, at another origin in every scene
        step = 3 if N >= 64 else 1
        if step == 1:
            boxes[b, 0, 0] += ORIGINS[b % 3]
        for i in range(step, A):
            place(b, i, i - step, gen.uniform(-0.4, 0.4))
        per_row = np.zeros(A, int)
        for n, j in enumerate(range(A, N)):
            i = n % A
            if per_row[i] >= 40:
                continue
            per_row[i] += 1
            place(b, j, i, gen.uniform(0.6, 2 * np.pi - 0.6))
    return boxes, present


def make(A, N, metric, name):
    """boxes (B, N, 5) float32 and present (B, N) bool of one case; deterministic"""
    B = batch_of(N)
    seed = [A, N, SETS.index(name), 0 if metric == 'iou' else 1]
    gen = np.random.default_rng(seed)
    boxes, present = dict(mixed=_mixed, ties=_ties, scrub=_scrub, rim=_rim)[name](gen, B, A, N)
    return boxes.astype(np.float32), present


def rim_counts(boxes, A):
    """(inside, outside): ordered pairs (i < A, j != i) within 2.5 mm of the cull threshold, by the side the float32 test puts them on"""
    B, N = boxes.shape[:2]
    b64 = boxes.astype(np.float64)
    inside = outside = 0
    for b in range(B):
        bi, bj = boxes[b, :A, None, :], boxes[b, None, :, :]
        d2, r2 = reach_f32(np.broadcast_to(bi, (A, N, 5)), np.broadcast_to(bj, (A, N, 5)))
        dist = np.hypot(b64[b, :A, None, 0] - b64[b, None, :, 0], b64[b, :A, None, 1] - b64[b, None, :, 1])
        close = np.abs(dist - np.sqrt(r2.astype(np.float64))) < 2.5e-3
        close &= np.arange(N)[None, :] != np.arange(A)[:, None]
        inside += int((close & ~(d2 > r2)).sum())
        outside += int((close & (d2 > r2)).sum())
    return inside, outside


def check_conditions(A, N, metric, name, boxes, present, m):
    """Is the input set what it claims to be?  Judged on the inputs and the model `m` (collision_model.model) alone, never on a kernel."""
    B = boxes.shape[0]
    rows = B * A
    collide = int((m['collision'] > 0).sum())
    tied = int(((m['ties'] >= 2) & (m['best'] > 0)).sum())
    if N == 1:
        assert collide == 0 and (m['partner'] == -1).all()           # a lone box: nothing to collide with
        return
    if name == 'mixed':
        assert rows / 4 <= collide <= 3 * rows / 4, (collide, rows)
        assert (boxes[..., 3] > boxes[..., 2]).any() or N < 8
        assert not present.all() or N < 8
    if name == 'ties' and N >= 7:
        assert tied >= min(5, rows), (tied, rows)                   # A = 1 and A = 2 have fewer than 5 rows: then every row is tied
        src = 1 if A >= 2 else 0                                     # the copies of an exposed agent overlap it as much as it overlaps itself
        assert (m['O'][:, src, N - 1] == m['O'][:, src, src]).all() and (m['O'][:, src, 3] == m['O'][:, src, src]).all()
    # a partner beyond the first chunk; in the ties set the tied rows must answer with the copy in the FIRST chunk, so a row of its own (6) does this where a second index >= 64 exists
    if N > 64 and (name in ('mixed', 'scrub') or (name == 'ties' and A >= 7 and N - 2 >= 64)):
        assert (m['partner'] >= 64).any()
    if name in ('mixed', 'ties') and N == 64:
        assert (m['bits'] >> np.uint64(63)).any()
    if name == 'ties' and N > 64:
        assert ((m['ties'] >= 2) & (m['partner'] < 64) & (m['partner'] >= 0)).any()   # a tie whose lowest member is in the first chunk
    if name == 'scrub':
        assert np.isnan(boxes[..., 0]).any() and (np.isnan(boxes[..., 4]).any() or N < 2) and (np.isnan(boxes[..., 2]).any() or N < 7)
        assert not present[:, :A].all() or N < 7
        assert collide > 0 or N < 7
    if name == 'rim':
        inside, outside = rim_counts(boxes, A)
        assert inside >= 20 and outside >= 20, (inside, outside)
