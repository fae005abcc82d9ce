"""
The yardstick of K2a's forward outputs (csrc/collision.hip, tds_collision_f32): the full A x N overlap matrix of a scene, built pair by pair
with the oracle's element-wise functions (oracle.iou_pairs / oracle.discs_pairs) and reduced with numpy.  Nothing of the product is used, and
there is no near-pair cull, no LDS list, no 64-lane chunk and no ballot in here, so it cannot share a bug with either kernel.

    boxes (B, N, 5) [x, y, length, width, psi], sc (B, N, 2) [sin, cos] of the angle the metric uses (the SAME values the kernel gets),
    present (B, N), A = number of exposed agents (the first A boxes), metric 'iou' | 'discs'

Steps, all float32 (simulator.py:1095-1108 of the reference):
    scrub       nan_to_num on the boxes; where psi is NaN the heading becomes 0, so [sin, cos] is that of the metric's angle of the scrubbed box:
                [0, 1], or for discs on a box wider than long [sin, cos](pi / 2)
    O[b,i,j]    = nan_to_num(pair(box_i, box_j)) * present_j over the full grid
    collision   = (sum over j in index order) - max_j
    bits        (N <= 64 only) uint64, bit j set iff O[b,i,j] > 0 and j != i
    partner     the LOWEST j != i that attains the largest O[b,i,j] > 0, else -1
"""
import numpy as np

F32_MAX = np.float32(3.4028234663852886e38)


def scrub_boxes(boxes, sc, metric):
    boxes = np.asarray(boxes, np.float32)
    sc = np.array(sc, np.float32)
    nan_psi = np.isnan(boxes[..., 4])
    b = np.nan_to_num(boxes, nan=0.0, posinf=F32_MAX, neginf=-F32_MAX).astype(np.float32)
    ang = np.zeros(b.shape[:-1], np.float32)
    if metric == 'discs':
        ang = np.where(b[..., 3] > b[..., 2], np.float32(np.pi) / np.float32(2.0), np.float32(0.0)).astype(np.float32)
    sc[nan_psi] = np.stack([np.sin(ang), np.cos(ang)], -1).astype(np.float32)[nan_psi]
    return b, sc


def overlap_matrix(boxes, sc, present, A, metric):
    """(B, A, N) float32: the scrubbed, masked overlaps"""
    from oracle import oracle as orc
    pair = dict(iou=orc.iou_pairs, discs=orc.discs_pairs)[metric]
    b, sc = scrub_boxes(boxes, sc, metric)
    B, N = b.shape[:2]
    O = np.zeros((B, A, N), np.float32)
    if A == 0 or N == 0:
        return O
    i, j = np.repeat(np.arange(A), N), np.tile(np.arange(N), A)
    for s in range(B):
        o = pair(b[s, i], b[s, j], sc[s, i], sc[s, j]).reshape(A, N)
        o = np.nan_to_num(o, nan=0.0, posinf=F32_MAX, neginf=-F32_MAX).astype(np.float32)
        O[s] = o * np.asarray(present[s], bool).astype(np.float32)[None, :]
    return O


def reduce_rows(O):
    """dict(collision (B,A) f32, partner (B,A) i32, best (B,A) f32 = the partner's overlap or 0, ties (B,A) = how many j != i attain it,
    bits (B,A) u64 or None)"""
    B, A, N = O.shape
    if N == 0:
        z = np.zeros((B, A), np.float32)
        return dict(collision=z, partner=np.full((B, A), -1, np.int32), best=z, ties=np.zeros((B, A), np.int64), bits=np.zeros((B, A), np.uint64))
    total = np.zeros((B, A), np.float32)
    for j in range(N):                                     # index order, one float32 rounding per addition
        total = (total + O[:, :, j]).astype(np.float32)
    collision = (total - O.max(-1)).astype(np.float32)
    other = np.arange(N)[None, :] != np.arange(A)[:, None]                 # j != i
    hit = (O > 0) & other[None]
    Oh = np.where(hit, O, np.float32(0.0))
    best = Oh.max(-1)
    at_best = hit & (Oh == best[..., None])
    partner = np.where(best > 0, at_best.argmax(-1), -1).astype(np.int32)   # argmax of a bool array: the first True
    bits = None
    if N <= 64:
        bits = (hit.astype(np.uint64) << np.arange(N, dtype=np.uint64)[None, None, :]).sum(-1, dtype=np.uint64)
    return dict(collision=collision, partner=partner, best=best, ties=at_best.sum(-1), bits=bits)


def model(boxes, sc, present, A, metric):
    O = overlap_matrix(boxes, sc, present, A, metric)
    r = reduce_rows(O)
    r['O'] = O
    return r
