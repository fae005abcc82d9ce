"""
Tensor-level entry points of the HIP kernels (device tensors in, device tensors out, launched on torch's current
stream through the C ABI of include/tdship.h).  The reference-shaped classes in kinematic.py, infractions.py,
rendering/ and simulator.py are thin layers over these.
"""
import atexit
import collections
import ctypes
import math
import sys
import threading

import numpy as np
import torch

from torchdrivesim_amd import _native as nat

f32, u8, i32 = torch.float32, torch.uint8, torch.int32


def _c(t, dtype=f32):
    """dense tensor of the dtype the kernels read (no copy when already so)"""
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _u8(mask):
    """a mask as the uint8 bytes the kernels read (a dense bool tensor is reinterpreted, not copied)"""
    return mask.contiguous().view(u8) if mask.dtype == torch.bool else _c(mask, u8)


def heading_sc(psi):
    """[sin, cos] of headings with torch on the tensor's device -- exactly where the reference calls torch.sin/cos
    (simulator.py:940, utils.py:40-53, _iou_utils.py:290-291).  psi: (...,) -> (..., 2); differentiable."""
    if psi.requires_grad and torch.is_grad_enabled():
        return torch.stack([torch.sin(psi), torch.cos(psi)], dim=-1)
    sc = torch.empty(psi.shape + (2,), dtype=psi.dtype, device=psi.device)          # two launches instead of three: the same torch.sin / torch.cos, written in place
    torch.sin(psi, out=sc[..., 0])
    torch.cos(psi, out=sc[..., 1])
    return sc


_zero_consts = {}


def _zeros_const(shape, device):
    """a zero tensor that is never written (gradient columns that are identically zero are concatenated from it: one launch, no fill).
    Cached per (shape, device) once it exists on the device for every stream: created outside stream capture only (a captured
    torch.zeros is a graph node in the graph's private pool, not memory an eager backward may read later) and followed by ONE
    synchronisation of the creating stream, so that a first use from another stream is ordered behind the fill."""
    dev = torch.device(device)
    if dev.type == 'cuda' and torch.cuda.is_current_stream_capturing():
        return torch.zeros(tuple(int(d) for d in shape), dtype=f32, device=dev)
    key = (tuple(int(d) for d in shape), str(dev))
    z = _zero_consts.get(key)
    if z is None:
        if len(_zero_consts) > 64:
            _zero_consts.clear()
        z = _zero_consts[key] = torch.zeros(key[0], dtype=f32, device=dev)
        if dev.type == 'cuda':
            torch.cuda.current_stream(dev).synchronize()
    return z


class _StateHeadingSC(torch.autograd.Function):
    """[sin psi, cos psi] of a (..., 4) state tensor as ONE autograd node.  The values are torch.sin / torch.cos of the psi column (what the
    reference computes, simulator.py:940); the backward is the chain rule in closed form, d/dpsi = g_sin cos - g_cos sin, written into the psi
    column of a zero state gradient -- three small launches instead of the eight of autograd's select / sin / cos / stack chain, and the
    consumers of one state (render, collision, off-road) can share the node (Simulator._heading_sc).  The node is shared, so it must be walkable
    more than once without retain_graph (autograd.grad of the collisions, then of the off-road loss: save_for_backward would free the values after
    the first walk) -- the values are kept on ctx, as a DETACHED ALIAS of the output: the output itself on ctx made the cycle
    output -> grad_fn -> ctx -> output, which only the cycle collector frees (GPU memory pressure does not wake it); the alias shares the
    storage and references nothing.  (An in-place edit of the returned tensor is therefore not caught by autograd's version check.)"""

    @staticmethod
    def forward(ctx, state):
        psi = state[..., 2]
        sc = torch.empty(state.shape[:-1] + (2,), dtype=state.dtype, device=state.device)
        torch.sin(psi, out=sc[..., 0])
        torch.cos(psi, out=sc[..., 1])
        ctx.sc = sc.detach()
        return sc

    @staticmethod
    def backward(ctx, g):
        sc = ctx.sc
        gpsi = torch.mul(g[..., 0], sc[..., 1]).addcmul_(g[..., 1], sc[..., 0], value=-1.0)
        z = _zeros_const(gpsi.shape + (2,), gpsi.device)
        return torch.cat([z, gpsi.unsqueeze(-1), z[..., :1]], dim=-1)          # (..., 4): zeros, zeros, d/dpsi, zeros


def state_heading_sc(state):
    """differentiable [sin psi, cos psi] of a (..., 4) state, one autograd node (see _StateHeadingSC)"""
    return _StateHeadingSC.apply(state)


class _Boxes(torch.autograd.Function):
    """[x, y, length, width, psi] boxes (simulator.py:1093) from a (..., 4) state and (..., 2) sizes as one autograd node: a cat forward, and a
    backward that builds both gradients with two launches instead of the zeros + copies + adds of three slice nodes."""

    @staticmethod
    def forward(ctx, state, size):
        ctx.need = (state.requires_grad, size.requires_grad)
        return torch.cat([state[..., :2], size, state[..., 2:3]], dim=-1)

    @staticmethod
    def backward(ctx, g):
        gs = gz = None
        if ctx.need[0]:
            gs = torch.cat([g[..., :2], g[..., 4:5], _zeros_const(g.shape[:-1] + (1,), g.device)], dim=-1)      # d/d(x, y, psi), 0 for v
        if ctx.need[1]:
            gz = g[..., 2:4].contiguous()
        return gs, gz


def state_boxes(state, size):
    return _Boxes.apply(state, size)


# ---------------------------------------------------------------------------------------------------------------
# K1 kinematics
# ---------------------------------------------------------------------------------------------------------------
class _BicycleStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, action, lr, dt, max_acc, max_steer, left_handed, no_reversing):
        state, action, lr = _c(state), _c(action), _c(lr)
        out = torch.empty_like(state)
        n = lr.numel()
        nat.call('tds_bicycle_step_f32', state.device, state, action, lr, out, n, dt, max_acc, max_steer, int(left_handed), int(no_reversing))
        ctx.save_for_backward(state, action, lr)
        ctx.cfg = (dt, max_acc, max_steer, int(left_handed), int(no_reversing))
        return out

    @staticmethod
    def backward(ctx, gout):
        state, action, lr = ctx.saved_tensors
        dt, max_acc, max_steer, lh, norev = ctx.cfg
        gout = _c(gout)
        gs, ga, gl = torch.empty_like(state), torch.empty_like(action), torch.empty_like(lr)
        nat.call('tds_bicycle_step_bwd_f32', state.device, state, action, lr, gout, gs, ga, gl, lr.numel(), dt, max_acc, max_steer, lh, norev)
        return gs, ga, gl, None, None, None, None, None


def bicycle_step(state, action, lr, dt=0.1, max_acc=5.0, max_steer=float(np.float32(np.pi / 2)), left_handed=False,
                 no_reversing=False):
    """state (...,4), action (...,2), lr (...) -> new state tensor (...,4) (kinematic.py:462-477 / :513-523)"""
    assert state.shape[-1] == 4 and action.shape[-1] == 2 and state.shape[:-1] == action.shape[:-1] == lr.shape
    return _BicycleStep.apply(state, action, lr, float(dt), float(max_acc), float(max_steer), bool(left_handed), bool(no_reversing))


class _SimpleStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, action, dt, norm, oriented):
        state, action = _c(state), _c(action)
        out = torch.empty_like(state)
        cn = (ctypes.c_float * 4)(*norm)
        nat.call('tds_simple_step_f32', state.device, state, action, out, state.numel() // 4, dt, cn, int(oriented))
        ctx.save_for_backward(state, action)
        ctx.cfg = (dt, tuple(norm), int(oriented))
        return out

    @staticmethod
    def backward(ctx, gout):
        state, action = ctx.saved_tensors
        dt, norm, oriented = ctx.cfg
        gout = _c(gout)
        gs, ga = torch.empty_like(state), torch.empty_like(action)
        cn = (ctypes.c_float * 4)(*norm)
        nat.call('tds_simple_step_bwd_f32', state.device, state, action, gout, gs, ga, state.numel() // 4, dt, cn, oriented)
        return gs, ga, None, None, None


def simple_step(state, action, dt=0.1, norm=(20.0, 20.0, 10 * np.pi, 5.0), oriented=False):
    assert state.shape[-1] == 4 and action.shape == state.shape
    return _SimpleStep.apply(state, action, float(dt), tuple(float(x) for x in norm), bool(oriented))


class _UnicycleStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, action, dt, max_acc, max_w):
        state, action = _c(state), _c(action)
        out = torch.empty_like(state)
        nat.call('tds_unicycle_step_f32', state.device, state, action, out, state.numel() // 4, dt, max_acc, max_w)
        ctx.save_for_backward(state, action)
        ctx.cfg = (dt, max_acc, max_w)
        return out

    @staticmethod
    def backward(ctx, gout):
        state, action = ctx.saved_tensors
        dt, max_acc, max_w = ctx.cfg
        gout = _c(gout)
        gs, ga = torch.empty_like(state), torch.empty_like(action)
        nat.call('tds_unicycle_step_bwd_f32', state.device, state, action, gout, gs, ga, state.numel() // 4, dt, max_acc, max_w)
        return gs, ga, None, None, None


def unicycle_step(state, action, dt=0.1, max_acc=5.0, max_yaw_rate=1.0):
    assert state.shape[-1] == 4 and action.shape[-1] == 2
    return _UnicycleStep.apply(state, action, float(dt), float(max_acc), float(max_yaw_rate))


# ---------------------------------------------------------------------------------------------------------------
# K2a collisions
# ---------------------------------------------------------------------------------------------------------------
_METRICS = {'iou': nat.METRIC_IOU, 'discs': nat.METRIC_DISCS}


def metric_sc(boxes, metric):
    """[sin, cos] of the heading the metric uses: psi (iou, _iou_utils.py:290-291) or
    psi + pi/2 * (width > length) (discs, infractions.py:404).  boxes (...,5)."""
    psi = boxes[..., 4]
    if metric == 'discs':
        psi = psi + (np.pi / 2) * (boxes[..., 3] > boxes[..., 2])
    return heading_sc(psi)


def collision_forward(boxes, sc, present, n_exposed, metric, want_overlap=False, want_partner=False):
    boxes, sc = _c(boxes), _c(sc)
    present = _u8(present)
    B, N = boxes.shape[:2]
    A = N if n_exposed is None else int(n_exposed)
    out = torch.empty((B, A), dtype=f32, device=boxes.device)
    overlap = torch.empty((B, A), dtype=torch.int64, device=boxes.device) if want_overlap else None
    partner = torch.empty((B, A), dtype=i32, device=boxes.device) if want_partner else None
    nat.call('tds_collision_f32', boxes.device, boxes, sc, present, out, overlap, partner, B, A, N, _METRICS[metric])
    return out, overlap, partner


def overlap_count(boxes, present, sc=None):
    """The `nograd` collision metric (simulator.py:1111-1149, infractions.py:352-375): boxes (B,A,5), present (B,A) -> (B,A) float64,
    the number of other present agents whose rectangle shares area with the agent's.  NaNs are scrubbed to 0 first."""
    boxes = torch.nan_to_num(_c(boxes.detach()), nan=0.0)
    sc = heading_sc(boxes[..., 4]) if sc is None else _c(sc)
    present = _u8(present)
    B, A = boxes.shape[:2]
    out = torch.empty((B, A), dtype=torch.float64, device=boxes.device)
    nat.call('tds_overlap_count_f32', boxes.device, boxes, sc, present, out, B, A)
    return out


class _Collision(torch.autograd.Function):
    @staticmethod
    def forward(ctx, boxes, sc, present, n_exposed, metric):
        boxes, sc = _c(boxes), _c(sc)
        out, _, _ = collision_forward(boxes, sc, present, n_exposed, metric)
        ctx.save_for_backward(boxes, sc, present)
        ctx.cfg = (n_exposed, metric)
        return out

    @staticmethod
    def backward(ctx, gout):
        boxes, sc, present = ctx.saved_tensors
        n_exposed, metric = ctx.cfg
        B, N = boxes.shape[:2]
        A = N if n_exposed is None else int(n_exposed)
        gout = _c(gout)
        pres = _u8(present)
        gb, gsc = torch.empty_like(boxes), torch.empty_like(sc)
        nat.call('tds_collision_bwd_f32', boxes.device, boxes, sc, pres, gout, gb, gsc, B, A, N, _METRICS[metric])
        return gb, gsc, None, None, None


def collision(boxes, present, n_exposed=None, metric='iou', sc=None):
    """Simulator.compute_collision fused over a scene: boxes (B,N,5) [x,y,len,wid,psi], present (B,N) -> (B,A)."""
    if sc is None:
        sc = metric_sc(torch.nan_to_num(boxes, nan=0.0), metric)
    return _Collision.apply(boxes, sc, present, n_exposed, metric)


def pairwise_overlap(box1, box2, metric='iou', sc1=None, sc2=None, num_discs=5):
    """iou_differentiable / collision_detection_with_discs (infractions.py:307,503), element-wise; boxes (...,5).
    Forward only (the fused scene entry point carries the gradient)."""
    shape = box1.shape[:-1]
    if sc1 is None:
        sc1 = metric_sc(box1, metric)
    if sc2 is None:
        sc2 = metric_sc(box2, metric)
    b1, b2, s1, s2 = _c(box1).reshape(-1, 5), _c(box2).reshape(-1, 5), _c(sc1).reshape(-1, 2), _c(sc2).reshape(-1, 2)
    out = torch.empty(b1.shape[0], dtype=f32, device=b1.device)
    if metric == 'discs' and num_discs != 5:
        nat.call('tds_pairwise_discs_f32', b1.device, b1, s1, b2, s2, out, b1.shape[0], int(num_discs))
    else:
        nat.call('tds_pairwise_overlap_f32', b1.device, b1, s1, b2, s2, out, b1.shape[0], _METRICS[metric])
    return out.reshape(shape)


def box2corners(box, sc=None):
    """_iou_utils.box2corners_th: (...,5) -> (...,4,2)"""
    if sc is None:
        sc = heading_sc(box[..., 4])
    b, s = _c(box).reshape(-1, 5), _c(sc).reshape(-1, 2)
    out = torch.empty((b.shape[0], 4, 2), dtype=f32, device=b.device)
    nat.call('tds_box2corners_f32', b.device, b, s, out, b.shape[0])
    return out.reshape(box.shape[:-1] + (4, 2))


# ---------------------------------------------------------------------------------------------------------------
# static map handle, K2b offroad
# ---------------------------------------------------------------------------------------------------------------
def occlusion_mask(state, size, present, n_exposed):
    """StandardSensingObservationNoise.get_noisy_present_mask (observation_noise.py:89-132): state (B,E,4), size (B,E,2),
    present (B,E) -> (B,A,E) bool, True = present and in line of sight of ego a"""
    B, E = present.shape
    state, size = _c(state.detach()), _c(size.detach())
    p8 = _u8(present)
    out = torch.empty((B, int(n_exposed), E), dtype=u8, device=state.device)
    nat.call('tds_occlusion_mask_f32', state.device, state, size, p8, out, B, int(n_exposed), E)
    return out.view(torch.bool)


def quantise_colors(attrs):
    """cv2.py:50: floor(attr * (1 - 1e-3) * 256) as uint8, packed 0x00RRGGBB.  attrs (...,3) float32 cpu tensor -> int64"""
    q = (attrs.to(f32) * (1.0 - 1e-3) * 256).floor().to(torch.uint8).to(torch.int64)
    return (q[..., 0] << 16) | (q[..., 1] << 8) | q[..., 2]


class _Handle:
    """A native object of the library (`_h`, on `self.device`) that the entry point named by `_destroy_call` destroys: at close(), or when
    the wrapper goes."""
    _destroy_call = None

    @property
    def handle(self):
        if self._h is None:
            raise RuntimeError(f'{type(self).__name__} was destroyed')
        return self._h

    def _destroy(self):
        if getattr(self, '_h', None) is not None:
            h, self._h = self._h, None
            nat.call(self._destroy_call, self.device, h)

    def close(self):
        self._destroy()

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass


class StaticMap(_Handle):
    """Device-resident static mesh + uniform grid (tds_map_t).  Built once per map and per device from HOST arrays."""
    _destroy_call, _keys_call = 'tds_map_destroy', 'tds_map_keys'

    def __init__(self, verts, faces, face_z=None, face_rgb=None, levels=None, device='cuda', cell_size=0.0):
        verts = np.ascontiguousarray(torch.as_tensor(verts).detach().cpu().numpy(), dtype=np.float32).reshape(-1, 2)
        faces = np.ascontiguousarray(torch.as_tensor(faces).detach().cpu().numpy(), dtype=np.int32).reshape(-1, 3)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('StaticMap lives on an MI355X; there is no CPU implementation')
        self.n_verts, self.n_faces = verts.shape[0], faces.shape[0]
        self.levels = None if levels is None else [float(x) for x in levels]
        vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        fz = None if face_z is None else np.ascontiguousarray(np.asarray(face_z), dtype=np.float32)
        fc = None if face_rgb is None else np.ascontiguousarray(np.asarray(face_rgb), dtype=np.uint32)
        lv = None if levels is None else np.ascontiguousarray(np.asarray(levels), dtype=np.float32)
        handle = ctypes.c_void_p()
        global map_creations
        map_creations += 1
        nat.call('tds_map_create', self.device, vp(verts), vp(faces), vp(fz), vp(fc), verts.shape[0], faces.shape[0], vp(lv),
                 0 if lv is None else len(lv), float(cell_size), ctypes.byref(handle))
        self._h = handle

    def face_keys(self):
        """distinct face keys of the map, or over the maps of a set (None: more than 64) -- with the actors' keys they decide which
        rasteriser serves a launch"""
        if not hasattr(self, '_face_keys'):
            buf, n = (ctypes.c_uint32 * 64)(), ctypes.c_int(0)
            nat.call(self._keys_call, self.device, self.handle, ctypes.cast(buf, ctypes.c_void_p), 64, ctypes.byref(n))
            self._face_keys = None if n.value < 0 else [int(buf[i]) for i in range(n.value)]
        return self._face_keys

    def info(self):
        buf = (ctypes.c_int64 * 10)()
        nat.call('tds_map_info_ex', self.device, self.handle, buf, 10)
        return dict(V=buf[0], F=buf[1], nx=buf[2], ny=buf[3], entries=buf[4], bytes=buf[5], n_levels=buf[6], near_candidates=buf[7],
                    render_entries=buf[8], pairs=buf[9])

    def rank_of(self, level):
        """1-based painter rank of a rendering level (larger = drawn later = on top)"""
        return self.levels.index(float(level)) + 1

    def close(self):
        """destroy the device map now -- unless the process-wide cache handed it out (`shared`): other simulators may hold it, and it is
        destroyed when the last holder drops it"""
        if not getattr(self, 'shared', False):
            self._destroy()


#: how many tds_map_create calls this process has made (tests count them: one per DISTINCT mesh, none for a batch operation)
map_creations = 0

_ROW_SEEDS = (0x9e3779b97f4a7c15, 0xc2b2ae3d27d4eb4f)


def _rows_view(t):
    """(tensor to read, number of rows, bytes per row, bytes between rows) for the row kernels: whole 4-byte words, dense inside a row;
    a batch that is ONE row expanded (stride 0) is one row.  Rows are compared by their bits."""
    if t.dim() == 0:
        raise RuntimeError('group_rows needs tensors with a leading batch axis')
    if t.dtype in (torch.bool, torch.uint8, torch.int8, torch.int16, torch.float16, torch.bfloat16):
        # narrower than a word: every element widened to one word of its own.  The BITS are widened, not the values -- a value conversion
        # of half-precision numbers truncates them (0.3 and 0.9 are both 0), and rows that differ only in fractional parts would share a map
        t = t.view(torch.int16 if t.element_size() == 2 else torch.uint8).to(torch.int32)
    n = t.shape[0]
    if n > 1 and t.stride(0) == 0:
        t, n = t[:1], 1
    if not t.is_contiguous():                      # (rows a stride apart too: the entry points take them, the binding's check of `rows` does not)
        t = t.contiguous()
    row_bytes = (t[0].numel() if n else 0) * t.element_size()
    stride = t.stride(0) * t.element_size() if n > 1 else row_bytes
    return t, n, row_bytes, stride


def row_hashes(tensors):
    """(B, 2 * len(tensors)) int64 device tensor: two 64-bit content hashes of every batch row of every tensor (tds_rows_hash_u64).  A batch
    that is one row expanded is hashed once and the hash repeated."""
    B = tensors[0].shape[0]
    dev = tensors[0].device
    cols = []
    for t in tensors:
        if t.shape[0] != B:
            raise RuntimeError('row_hashes: the tensors do not share the batch axis')
        v, n, row_bytes, stride = _rows_view(t.detach())
        for seed in _ROW_SEEDS:
            h = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
            if n:
                nat.call('tds_rows_hash_u64', dev, v, n, row_bytes, stride, seed, h)
            cols.append(h[:n].expand(B) if n != B else h)
    return torch.stack(cols, dim=1) if cols else torch.zeros(B, 0, dtype=torch.int64, device=dev)


def group_rows(tensors):
    """Which batch elements of the (device) tensors are identical in ALL of them -- the scenes of a collated batch that share a mesh
    (mesh.py:172-200: padded rows of the same map are identical byte for byte).  Returns (scene_map, reps, hashes):
        scene_map  (B,) numpy int32, group of every batch element, groups numbered by first occurrence;
        reps       list, the first batch element of every group;
        hashes     list of tuples, the content hashes of every group's rows (keys of the process-wide map cache).
    Grouping is by hash on the device, then CONFIRMED exactly (tds_rows_equal_u8 against the group's representative); a row that shares a
    hash but not the bytes becomes a group of its own.  One small device -> host copy (B hashes); the meshes stay on the device."""
    B = tensors[0].shape[0]
    if B == 0:
        return np.zeros(0, np.int32), [], []
    dev = tensors[0].device
    h = row_hashes(tensors).cpu().numpy()                                         # B x 2T
    index, reps, scene_map = {}, [], np.empty(B, np.int32)
    for b in range(B):
        key = h[b].tobytes()
        g = index.get(key)
        if g is None:
            g = index[key] = len(reps)
            reps.append(b)
        scene_map[b] = g
    if len(reps) < B:
        rep = torch.from_numpy(np.asarray(reps, np.int32)[scene_map]).to(dev)
        equal = torch.ones(B, dtype=u8, device=dev)
        for t in tensors:
            v, n, row_bytes, stride = _rows_view(t.detach())
            if n == B:
                nat.call('tds_rows_equal_u8', dev, v, n, row_bytes, stride, rep, equal)
        bad = np.nonzero(equal.cpu().numpy() == 0)[0]
        for b in bad:                                                            # a hash collision: the row gets a map of its own
            scene_map[b] = len(reps)
            reps.append(int(b))
    hashes = [tuple(int(x) for x in h[r]) for r in reps]
    return scene_map, reps, hashes


class MapCache:
    """Process-wide cache of device maps by CONTENT: (device, what the map was built for, content hashes of the mesh rows, parameters) ->
    StaticMap, with the rows it was built from kept beside it (device clones, about a megabyte per map) so that a hit is confirmed byte for
    byte.  Maps are immutable, so simulators, their copies, sub-batches (`select_batch_elements`), extensions and shards share handles
    instead of running tds_map_create again (the reference carries B private mesh copies through these operations, simulator.py:444-511).
    Least recently used entries are dropped beyond `capacity` maps (TDS_MAP_CACHE, default 64); a dropped map lives on while a simulator
    holds it."""

    def __init__(self, capacity=None):
        import os
        self.capacity = int(os.environ.get('TDS_MAP_CACHE', 64)) if capacity is None else capacity
        self._d = collections.OrderedDict()
        self._lock = threading.Lock()
        self.hits = self.misses = 0

    def get(self, key, rows, build):
        """the cached map of `key` if its stored rows equal `rows` (list of device tensors), else build() -> StaticMap, stored"""
        key = (key, id(nat.lib()))             # (the testing build is a separate image of the library: its handles stay with it)
        with self._lock:
            ent = self._d.get(key)
            if ent is not None:
                smap, kept = ent
                if smap._h is not None and len(kept) == len(rows) and all(a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a, b)) for a, b in zip(kept, rows)):
                    self._d.move_to_end(key)
                    self.hits += 1
                    return smap
            self.misses += 1
            smap = build()
            smap.shared = True
            self._d[key] = (smap, [r.detach().clone() for r in rows])
            self._d.move_to_end(key)
            while len(self._d) > max(self.capacity, 0):
                self._d.popitem(last=False)
            return smap

    def clear(self):
        with self._lock:
            self._d.clear()


map_cache = MapCache()
atexit.register(map_cache.clear)


def map_per_distinct_row(tensors, prepare):
    """The device map of a batch of meshes: ONE StaticMap per distinct batch element of the (device) `tensors` (`group_rows`), each taken
    from the process-wide `map_cache` or built once.  prepare(reps) -> (key, build), called once per batch with the representatives:
    key(h, rows) is the cache key of the map of the representative whose content hashes are `h` and whose rows are `rows`, build(r) builds
    the map of batch element r.  Returns a StaticMap when the whole batch shares one mesh, else a StaticMapSet whose `scene_map` says
    which map scene b uses."""
    scene_map, reps, hashes = group_rows(tensors)
    key, build = prepare(reps)
    maps = []
    for r, h in zip(reps, hashes):
        rows = [t[r] for t in tensors]
        maps.append(map_cache.get(key(h, rows), rows, lambda r=r: build(r)))
    return maps[0] if len(maps) == 1 else StaticMapSet(maps, torch.from_numpy(scene_map))


class StaticMapSet(_Handle):
    """Several StaticMaps of one device (created with the same level table) + which of them every scene of a batch uses: lets one
    launch serve a batch whose scenes have different meshes (tds_mapset_t).  `scene_map`: (B,) int32 device tensor of indices."""
    _destroy_call, _keys_call = 'tds_mapset_destroy', 'tds_mapset_keys'
    face_keys = StaticMap.face_keys

    def __init__(self, maps, scene_map):
        assert len(maps) > 0
        self.maps = list(maps)                       # keeps the maps alive
        self.device = self.maps[0].device
        self.levels = self.maps[0].levels
        self.n_faces = sum(m.n_faces for m in self.maps)
        self.scene_map = _c(torch.as_tensor(scene_map).to(self.device), i32)
        arr = (ctypes.c_void_p * len(self.maps))(*[m.handle for m in self.maps])
        handle = ctypes.c_void_p()
        nat.call('tds_mapset_create', self.device, arr, len(self.maps), ctypes.byref(handle))
        self._h = handle

    def rank_of(self, level):
        return self.maps[0].rank_of(level)


def _agents_per_scene(smap, state):
    n_scenes = smap.scene_map.shape[0]
    n = state.numel() // 4
    if state.dim() < 2 or state.shape[0] != n_scenes or n % n_scenes:
        raise RuntimeError(f'a StaticMapSet for {n_scenes} scenes needs agent tensors of shape ({n_scenes}, A, ...), got {tuple(state.shape)}')
    return n // n_scenes


def _map_head(fn, suffix, smap, dev, agents=None):
    """the start of a call that takes one map or a map set: entry point, device, handle -- for a StaticMapSet the _multi form, whose handle is
    followed by the scene map and, where the entry point takes it (`agents`: the agent tensor), the agents per scene"""
    if isinstance(smap, StaticMapSet):
        return (fn + '_multi' + suffix, dev, smap.handle, smap.scene_map) + (() if agents is None else (_agents_per_scene(smap, agents),))
    return fn + suffix, dev, None if smap is None else smap.handle


def offroad_forward(smap, state, lenwid, sc, present, threshold):
    state, lenwid, sc = _c(state), _c(lenwid), _c(sc)
    n = state.numel() // 4
    out = torch.empty(state.shape[:-1], dtype=f32, device=state.device)
    pres = None if present is None else _u8(present)
    nat.call(*_map_head('tds_offroad', '_f32', smap, state.device, state), state, lenwid, sc, pres, out, n, float(threshold))
    return out


class _Offroad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, smap, state, lenwid, sc, present, threshold):
        state, lenwid, sc = _c(state), _c(lenwid), _c(sc)
        out = offroad_forward(smap, state, lenwid, sc, present, threshold)
        ctx.save_for_backward(state, lenwid, sc)
        ctx.cfg = (smap, present, threshold)
        return out

    @staticmethod
    def backward(ctx, gout):
        state, lenwid, sc = ctx.saved_tensors
        smap, present, threshold = ctx.cfg
        gout = _c(gout)
        pres = None if present is None else _u8(present)
        gs, gl, gsc = torch.empty_like(state), torch.empty_like(lenwid), torch.empty_like(sc)
        nat.call(*_map_head('tds_offroad', '_bwd_f32', smap, state.device, state), state, lenwid, sc, pres, gout, gs, gl, gsc, state.numel() // 4, float(threshold))
        return None, gs, gl, gsc, None, None


def offroad(smap, state, lenwid, threshold=0.5, present=None, sc=None):
    """offroad_infraction_loss (infractions.py:176-229, pure path) [* present]: state (...,4), lenwid (...,2) -> (...)"""
    if sc is None:
        sc = heading_sc(state[..., 2])
    return _Offroad.apply(smap, state, lenwid, sc, present, float(threshold))


# ---------------------------------------------------------------------------------------------------------------
# K5 range scans
# ---------------------------------------------------------------------------------------------------------------
def check_range_scan_args(n_rays, max_range, gap_tolerance):
    """the argument rules of tds_range_scan_f32, on the host: raised before anything is computed or launched"""
    if int(n_rays) != n_rays or int(n_rays) <= 0 or int(n_rays) > 65536:
        raise ValueError(f'range scan: the number of rays must be 1 .. 65536 (got {n_rays})')
    for name, v in (('max_range', max_range), ('gap_tolerance', gap_tolerance)):
        v = float(v)
        if not (0.0 <= v <= 3.0e38):                    # (finite as a float32 too; NaN fails both comparisons)
            raise ValueError(f'range scan: {name} must be finite and not negative (got {v})')


def range_scan(smap, boxes, sc, present, ray_sc, n_exposed, max_range, gap_tolerance, want_agents=True):
    """Range scan of every exposed agent (tds_range_scan_f32 / _multi, include/tdship.h "K5"): boxes (B,E,5) [x,y,length,width,psi], sc (B,E,2)
    [sin, cos] of psi, present (B,E), ray_sc (B,A,R,2) [sin, cos] of every ray -> (agents, road, hit), each (B,A,R): float32, float32, int32.
    smap: a StaticMap, a StaticMapSet (scene b on map scene_map[b]) or None (no road part: road = max_range).  want_agents=False skips the
    rectangles (agents = max_range).  No gradient; CPU tensors raise (there is no CPU fallback)."""
    if ray_sc.dim() != 4 or ray_sc.shape[-1] != 2:
        raise ValueError(f'range scan: ray_sc must be (B, A, R, 2), got {tuple(ray_sc.shape)}')
    B, A, R = (int(d) for d in ray_sc.shape[:3])
    check_range_scan_args(R, max_range, gap_tolerance)
    if boxes.dim() != 3 or boxes.shape[-1] != 5 or boxes.shape[0] != B:
        raise ValueError(f'range scan: boxes must be ({B}, E, 5), got {tuple(boxes.shape)}')
    E = int(boxes.shape[1])
    if int(n_exposed) != A or A > E:
        raise ValueError(f'range scan: {n_exposed} exposed agents, rays for {A}, {E} entities')
    if tuple(sc.shape) != (B, E, 2) or tuple(present.shape) != (B, E):
        raise ValueError(f'range scan: sc must be ({B}, {E}, 2) and present ({B}, {E}), got {tuple(sc.shape)} and {tuple(present.shape)}')
    boxes, sc, ray_sc = _c(boxes.detach()), _c(sc.detach()), _c(ray_sc.detach())
    present = _u8(present)
    dev = boxes.device
    if smap is not None and smap.device != dev:
        raise RuntimeError(f'range scan: the map lives on {smap.device}, the agents on {dev}')
    if isinstance(smap, StaticMapSet) and smap.scene_map.shape[0] != B:
        raise RuntimeError(f'range scan: a StaticMapSet for {smap.scene_map.shape[0]} scenes, agents of {B}')
    agents = torch.empty((B, A, R), dtype=f32, device=dev) if want_agents else None
    road = torch.empty((B, A, R), dtype=f32, device=dev)
    hit = torch.empty((B, A, R), dtype=i32, device=dev)
    nat.call(*_map_head('tds_range_scan', '_f32', smap, dev), boxes, sc, present, ray_sc, agents, road, hit, B, A, E, R, float(max_range), float(gap_tolerance))
    if agents is None:
        agents = torch.full((B, A, R), float(max_range), dtype=f32, device=dev)
    return agents, road, hit


def _range_scan_bwd(smap, boxes, sc, present, ray_sc, road, g_agent, g_road, want_grads, want_witness, max_range, gap_tolerance):
    """one call of tds_range_scan_bwd_f32 / _multi (include/tdship.h "K5b") -> g_boxes, g_sc, g_ray_sc, choice, road_edge (None where not asked for;
    want_witness = 'road': the road edge alone).  A part whose incoming gradient is None is skipped in the kernel; so is the road part without a map."""
    B, A, R = (int(d) for d in ray_sc.shape[:3])
    E = int(boxes.shape[1])
    dev = boxes.device
    g_boxes = torch.empty((B, E, 5), dtype=f32, device=dev) if want_grads else None
    g_sc = torch.empty((B, E, 2), dtype=f32, device=dev) if want_grads else None
    g_ray_sc = torch.empty((B, A, R, 2), dtype=f32, device=dev) if want_grads else None
    choice = torch.empty((B, A, R, 2), dtype=i32, device=dev) if want_witness and want_witness != 'road' else None
    road_edge = torch.empty((B, A, R, 4), dtype=f32, device=dev) if want_witness else None
    nat.call(*_map_head('tds_range_scan_bwd', '_f32', smap, dev), boxes, sc, present, ray_sc, road if smap is not None else None,
             None if g_agent is None else _c(g_agent), None if g_road is None or smap is None else _c(g_road), g_boxes, g_sc, g_ray_sc, choice, road_edge,
             B, A, E, R, float(max_range), float(gap_tolerance))
    return g_boxes, g_sc, g_ray_sc, choice, road_edge


class _RangeScanGrad(torch.autograd.Function):
    """K5 as an autograd node: forward = range_scan, backward = tds_range_scan_bwd_f32 / _multi (csrc/scan_bwd.hip), one launch"""

    @staticmethod
    def forward(ctx, smap, boxes, sc, present, ray_sc, n_exposed, max_range, gap_tolerance, want_agents):
        agents, road, hit = range_scan(smap, boxes, sc, present, ray_sc, n_exposed, max_range, gap_tolerance, want_agents=want_agents)
        ctx.mark_non_differentiable(hit)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(boxes, sc, present, ray_sc, road)
        ctx.cfg = (smap, float(max_range), float(gap_tolerance), bool(want_agents))
        return agents, road, hit

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_agent, g_road, _g_hit):
        smap, max_range, gap_tolerance, want_agents = ctx.cfg
        need = ctx.needs_input_grad
        if not want_agents:
            g_agent = None                                   # agents = max_range everywhere: a constant
        if smap is None:
            g_road = None                                    # road = max_range everywhere
        if (g_agent is None and g_road is None) or not (need[1] or need[2] or need[4]):
            return (None,) * 9
        boxes, sc, present, ray_sc, road = ctx.saved_tensors
        g_boxes, g_sc, g_ray_sc, _, _ = _range_scan_bwd(smap, _c(boxes.detach()), _c(sc.detach()), _u8(present), _c(ray_sc.detach()), road, g_agent, g_road,
                                                        True, False, max_range, gap_tolerance)
        return (None, g_boxes.to(boxes.dtype) if need[1] else None, g_sc.to(sc.dtype) if need[2] else None, None,
                g_ray_sc.to(ray_sc.dtype) if need[4] else None, None, None, None, None)


def range_scan_grad(smap, boxes, sc, present, ray_sc, n_exposed, max_range, gap_tolerance, want_agents=True):
    """`range_scan`, differentiable (include/tdship.h "K5b"): the same launch and the same bits; `agents` and `road` carry the graph
    to `boxes` ([x, y, length, width]; the psi column gets zeros -- psi has its gradient through `sc` and `ray_sc`), to `sc` = [sin psi, cos psi] of
    the entity a ray ends on and to `ray_sc`, `hit` never does.  The backward is ONE launch (tds_range_scan_bwd_f32 / _multi); a part that was not
    computed (want_agents=False, no map) is skipped in the kernel.  Constants of differentiation: the entity and the rectangle side that define
    `agents`, the road edge `road` ends on, the map, `max_range`, `gap_tolerance`.  A ray that is capped at `max_range`, starts inside a rectangle
    or off the road, or belongs to an absent agent contributes exactly zero whatever its incoming gradient holds.  No double backward."""
    return _RangeScanGrad.apply(smap, boxes, sc, present, ray_sc, n_exposed, max_range, gap_tolerance, want_agents)


def range_scan_witness(smap, boxes, sc, present, ray_sc, n_exposed, max_range, gap_tolerance, want_agents=True):
    """What the backward of `range_scan_grad` differentiates, from the same entry point with every gradient pointer NULL -> (choice (B,A,R,2) int32
    [the entity that defines `agents` or -1, the side that binds: 0 none, 1 length, 2 width], road_edge (B,A,R,4) float32 [x_i, y_i, x_j, y_j] of
    the road edge `road` ends on, NaN where the road contributes nothing)."""
    _, road, _ = range_scan(smap, boxes, sc, present, ray_sc, n_exposed, max_range, gap_tolerance, want_agents=False)
    B, A, R = road.shape
    _, _, _, choice, road_edge = _range_scan_bwd(smap, _c(boxes.detach()), _c(sc.detach()), _u8(present), _c(ray_sc.detach()), road, None, None, False,
                                                 True if want_agents else 'road', max_range, gap_tolerance)
    if not want_agents:
        choice = torch.stack([torch.full((B, A, R), -1, dtype=i32, device=road.device), torch.zeros((B, A, R), dtype=i32, device=road.device)], -1)
    return choice, road_edge


# ---------------------------------------------------------------------------------------------------------------
# K6 neighbour observations
# ---------------------------------------------------------------------------------------------------------------
def _check_k(what, k, limit):
    if int(k) != k or int(k) < 1 or int(k) > limit:
        raise ValueError(f'{what}: k must be 1 .. {limit} (got {k})')


def _check_reach(what, name, value):
    if not float(value) >= 0.0:                         # (NaN fails the comparison; +inf is allowed)
        raise ValueError(f'{what}: {name} must not be negative or NaN (got {value})')


def _entity_inputs(what, boxes, sc, speed, present, n_exposed, visible):
    """the entities of K6 and K9, checked and as the kernels read them -> boxes, sc, speed, present, visible, B, A, E"""
    if boxes.dim() != 3 or boxes.shape[-1] != 5:
        raise ValueError(f'{what}: boxes must be (B, E, 5), got {tuple(boxes.shape)}')
    B, E = int(boxes.shape[0]), int(boxes.shape[1])
    A = int(n_exposed)
    if A < 0 or A > E:
        raise ValueError(f'{what}: {n_exposed} exposed agents, {E} entities')
    if tuple(sc.shape) != (B, E, 2) or tuple(speed.shape) != (B, E) or tuple(present.shape) != (B, E):
        raise ValueError(f'{what}: sc must be ({B}, {E}, 2), speed and present ({B}, {E}), got {tuple(sc.shape)}, {tuple(speed.shape)} and '
                         f'{tuple(present.shape)}')
    if visible is not None:
        if tuple(visible.shape) != (B, A, E):
            raise ValueError(f'{what}: visible must be ({B}, {A}, {E}), got {tuple(visible.shape)}')
        if visible.dtype not in (torch.bool, u8):
            raise ValueError(f'{what}: visible must be bool or uint8, got {visible.dtype}')
    return _c(boxes.detach()), _c(sc.detach()), _c(speed.detach()), _u8(present), None if visible is None else _u8(visible), B, A, E


def check_neighbors_args(k, max_distance):
    """the argument rules of tds_neighbors_f32, on the host: raised before anything is computed or launched"""
    _check_k('neighbors', k, nat.NEIGHBORS_MAX_K)
    _check_reach('neighbors', 'max_distance', max_distance)


def neighbors(boxes, sc, speed, present, n_exposed, k, max_distance, visible=None):
    """The k nearest other entities of every exposed agent (tds_neighbors_f32, include/tdship.h "K6"): boxes (B,E,5) [x,y,length,width,psi],
    sc (B,E,2) [sin, cos] of psi, speed (B,E), present (B,E), visible None or (B,A,E) bool / uint8 -> features (B,A,k,8) float32,
    index (B,A,k) int32.  No gradient; CPU tensors raise (there is no CPU fallback)."""
    check_neighbors_args(k, max_distance)
    boxes, sc, speed, present, visible, B, A, E = _entity_inputs('neighbors', boxes, sc, speed, present, n_exposed, visible)
    K = int(k)
    dev = boxes.device
    features = torch.empty((B, A, K, 8), dtype=f32, device=dev)
    index = torch.empty((B, A, K), dtype=i32, device=dev)
    nat.call('tds_neighbors_f32', dev, boxes, sc, speed, present, visible, features, index, B, A, E, K, float(max_distance))
    return features, index


class _NeighborsGrad(torch.autograd.Function):
    """K6 as an autograd node: forward = neighbors, backward = tds_neighbors_bwd_f32 (csrc/neighbors_bwd.hip), one launch"""

    @staticmethod
    def forward(ctx, boxes, sc, speed, present, n_exposed, k, max_distance, visible):
        features, index = neighbors(boxes, sc, speed, present, n_exposed, k, max_distance, visible=visible)
        ctx.mark_non_differentiable(index)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(boxes, sc, speed, index)
        return features, index

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_features, _g_index):
        if g_features is None or not any(ctx.needs_input_grad[:3]):
            return (None,) * 8
        boxes, sc, speed, index = ctx.saved_tensors
        B, A, K = index.shape
        E = boxes.shape[1]
        dev = boxes.device
        g_boxes = torch.empty((B, E, 5), dtype=f32, device=dev)
        g_sc = torch.empty((B, E, 2), dtype=f32, device=dev)
        g_speed = torch.empty((B, E), dtype=f32, device=dev)
        nat.call('tds_neighbors_bwd_f32', dev, _c(boxes.detach()), _c(sc.detach()), _c(speed.detach()), index, _c(g_features), g_boxes, g_sc, g_speed,
                 B, A, E, K)
        need = ctx.needs_input_grad
        return (g_boxes.to(boxes.dtype) if need[0] else None, g_sc.to(sc.dtype) if need[1] else None, g_speed.to(speed.dtype) if need[2] else None) + \
            (None,) * 5


def neighbors_grad(boxes, sc, speed, present, n_exposed, k, max_distance, visible=None):
    """`neighbors`, differentiable (include/tdship.h "K6b"): the same launch and the same bits; `features` carries the graph to
    `boxes` ([x, y, length, width]; the psi column gets zeros -- psi has its gradient through `sc`), to `sc` = [sin psi, cos psi] and to `speed`
    of both entities of every filled slot, `index` never does.  The backward is ONE launch (tds_neighbors_bwd_f32).  Which entity is in a slot,
    the `max_distance` cut, `visible` and the order of the slots are constants.  An empty slot contributes exactly zero whatever its incoming
    gradient holds; a filled slot whose inputs are not finite propagates what IEEE arithmetic gives.  No double backward."""
    return _NeighborsGrad.apply(boxes, sc, speed, present, n_exposed, k, max_distance, visible)


# ---------------------------------------------------------------------------------------------------------------
# K9 time to collision
# ---------------------------------------------------------------------------------------------------------------
def check_ttc_args(k, horizon, margin):
    """the argument rules of tds_time_to_collision_f32, on the host: raised before anything is computed or launched"""
    _check_k('time_to_collision', k, nat.TTC_MAX_K)
    _check_reach('time_to_collision', 'horizon', horizon)
    if not math.isfinite(float(margin)):
        raise ValueError(f'time_to_collision: margin must be finite (got {margin})')


def time_to_collision(boxes, sc, speed, present, n_exposed, k, horizon, margin=0.0, visible=None):
    """The k entities every exposed agent would touch first within `horizon` seconds at constant velocity and heading, and when
    (tds_time_to_collision_f32, include/tdship.h "K9"): boxes (B,E,5) [x,y,length,width,psi], sc (B,E,2) [sin, cos] of psi, speed (B,E),
    present (B,E), visible None or (B,A,E) bool / uint8 -> ttc (B,A,k) float32 (+inf in an empty slot), index (B,A,k) int32 (-1 there).
    No gradient; CPU tensors raise (there is no CPU fallback)."""
    check_ttc_args(k, horizon, margin)
    boxes, sc, speed, present, visible, B, A, E = _entity_inputs('time_to_collision', boxes, sc, speed, present, n_exposed, visible)
    K = int(k)
    dev = boxes.device
    ttc = torch.empty((B, A, K), dtype=f32, device=dev)
    index = torch.empty((B, A, K), dtype=i32, device=dev)
    nat.call('tds_time_to_collision_f32', dev, boxes, sc, speed, present, visible, ttc, index, B, A, E, K, float(horizon), float(margin))
    return ttc, index


class _TimeToCollisionGrad(torch.autograd.Function):
    """K9 as an autograd node: forward = time_to_collision, backward = tds_time_to_collision_bwd_f32 (csrc/ttc_bwd.hip), one launch"""

    @staticmethod
    def forward(ctx, boxes, sc, speed, present, n_exposed, k, horizon, margin, visible):
        ttc, index = time_to_collision(boxes, sc, speed, present, n_exposed, k, horizon, margin, visible=visible)
        ctx.mark_non_differentiable(index)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(boxes, sc, speed, index)
        ctx.margin = float(margin)
        return ttc, index

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_ttc, _g_index):
        if g_ttc is None or not any(ctx.needs_input_grad[:3]):
            return (None,) * 9
        boxes, sc, speed, index = ctx.saved_tensors
        B, A, K = index.shape
        E = boxes.shape[1]
        dev = boxes.device
        g_boxes = torch.empty((B, E, 5), dtype=f32, device=dev)
        g_sc = torch.empty((B, E, 2), dtype=f32, device=dev)
        g_speed = torch.empty((B, E), dtype=f32, device=dev)
        nat.call('tds_time_to_collision_bwd_f32', dev, _c(boxes.detach()), _c(sc.detach()), _c(speed.detach()), index, _c(g_ttc), g_boxes, g_sc, g_speed,
                 B, A, E, K, ctx.margin)
        need = ctx.needs_input_grad
        return (g_boxes.to(boxes.dtype) if need[0] else None, g_sc.to(sc.dtype) if need[1] else None, g_speed.to(speed.dtype) if need[2] else None) + \
            (None,) * 6


def time_to_collision_grad(boxes, sc, speed, present, n_exposed, k, horizon, margin=0.0, visible=None):
    """`time_to_collision`, differentiable (include/tdship.h "K9b"): the same launch and the same bits; `ttc` carries the graph to
    `boxes` ([x, y, length, width]; the psi column gets zeros -- psi has its gradient through `sc`), to `sc` = [sin psi, cos psi] and to `speed`,
    `index` never does.  The backward is ONE launch (tds_time_to_collision_bwd_f32).  The forward's discrete choices -- which entity is in a slot,
    the axis that binds, the signs -- are constants.  A slot contributes iff it is filled and its time is above 0; an empty slot and a pair that
    overlaps already contribute exactly zero whatever their incoming gradient holds.  No gradient to `margin` or `horizon`, no double backward."""
    return _TimeToCollisionGrad.apply(boxes, sc, speed, present, n_exposed, k, horizon, margin, visible)


# ---------------------------------------------------------------------------------------------------------------
# K7 traffic lights on the device (csrc/lights.hip)
# ---------------------------------------------------------------------------------------------------------------
def lights_step(tables, phase, remaining, state, time_to_change, dt, advance=True, mask=None):
    """tds_lights_step (include/tdship.h "K7"): tables = (duration MxP float64, next_phase MxP int32, n_phases M int32, colour MxPxN uint8); phase
    (B,M) int32, remaining (B,M) float64, state (B,N) int64 and time_to_change (B,N) float32 are updated IN PLACE and must be dense tensors of
    exactly those types; mask None or (B,) bool / uint8.  One launch on the current stream, no allocation, no synchronisation."""
    duration, next_phase, n_phases, colour = tables
    B, M = phase.shape
    P, N = duration.shape[1], state.shape[1]
    if tuple(duration.shape) != (M, P) or tuple(next_phase.shape) != (M, P) or tuple(n_phases.shape) != (M,) or tuple(colour.shape) != (M, P, N):
        raise ValueError(f'lights_step: tables of {tuple(duration.shape)}, {tuple(next_phase.shape)}, {tuple(n_phases.shape)} and {tuple(colour.shape)} '
                         f'for {M} machines and {N} lights')
    if tuple(remaining.shape) != (B, M) or tuple(state.shape) != (B, N) or tuple(time_to_change.shape) != (B, N):
        raise ValueError(f'lights_step: remaining must be ({B}, {M}), state and time_to_change ({B}, {N}), got {tuple(remaining.shape)}, '
                         f'{tuple(state.shape)} and {tuple(time_to_change.shape)}')
    if mask is not None and tuple(mask.shape) != (B,):
        raise ValueError(f'lights_step: mask must be ({B},), got {tuple(mask.shape)}')
    nat.call('tds_lights_step', phase.device, duration, next_phase, n_phases, colour, phase, remaining, state, time_to_change,
             None if mask is None else _u8(mask), B, M, P, N, ctypes.byref(ctypes.c_double(float(dt))), int(bool(advance)))


def lights_reset(tables, phase, remaining, scene_ids, seed, mask=None):
    """tds_lights_reset: every machine of the masked scenes to the beginning of its Philox-picked phase, in place; follow it with
    lights_step(advance=False).  scene_ids (B,) int64."""
    duration, _, n_phases, _ = tables
    B, M = phase.shape
    if tuple(remaining.shape) != (B, M) or tuple(scene_ids.shape) != (B,) or (mask is not None and tuple(mask.shape) != (B,)):
        raise ValueError(f'lights_reset: remaining must be ({B}, {M}), scene_ids and mask ({B},)')
    nat.call('tds_lights_reset', phase.device, n_phases, duration, phase, remaining, None if mask is None else _u8(mask), scene_ids, B, M,
             duration.shape[1], _seed64(seed))


def check_stop_lines_args(k, max_distance, min_cos):
    """the argument rules of tds_stop_lines_f32, on the host: raised before anything is computed or launched"""
    _check_k('stop lines', k, nat.STOP_LINES_MAX_K)
    _check_reach('stop lines', 'max_distance', max_distance)
    if min_cos is not None and float(min_cos) != float(min_cos):
        raise ValueError('stop lines: min_cos must not be NaN')


def stop_lines(agent_xy, agent_sc, agent_present, lines, line_sc, mask, state, time_to_change, k, max_distance, ahead_only=True, min_cos=None):
    """The k nearest stop lines of every exposed agent (tds_stop_lines_f32, include/tdship.h "K7"): agent_xy (B,A,2), agent_sc (B,A,2) [sin, cos],
    agent_present (B,A); lines (B,N,5) [x,y,length,width,psi], line_sc (B,N,2), mask (B,N), state (B,N) int64, time_to_change None or (B,N)
    -> features (B,A,k,8) float32, index (B,A,k) int32, state (B,A,k) int32.  No gradient; CPU tensors raise (there is no CPU fallback)."""
    check_stop_lines_args(k, max_distance, min_cos)
    if agent_xy.dim() != 3 or agent_xy.shape[-1] != 2 or lines.dim() != 3 or lines.shape[-1] != 5 or lines.shape[0] != agent_xy.shape[0]:
        raise ValueError(f'stop lines: agent_xy must be (B, A, 2) and lines (B, N, 5), got {tuple(agent_xy.shape)} and {tuple(lines.shape)}')
    B, A, N, K = int(agent_xy.shape[0]), int(agent_xy.shape[1]), int(lines.shape[1]), int(k)
    if tuple(agent_sc.shape) != (B, A, 2) or tuple(agent_present.shape) != (B, A):
        raise ValueError(f'stop lines: agent_sc must be ({B}, {A}, 2) and agent_present ({B}, {A}), got {tuple(agent_sc.shape)} and {tuple(agent_present.shape)}')
    if tuple(line_sc.shape) != (B, N, 2) or tuple(mask.shape) != (B, N) or tuple(state.shape) != (B, N) or \
            (time_to_change is not None and tuple(time_to_change.shape) != (B, N)):
        raise ValueError(f'stop lines: line_sc must be ({B}, {N}, 2), mask, state and time_to_change ({B}, {N})')
    dev = agent_xy.device
    features = torch.empty((B, A, K, 8), dtype=f32, device=dev)
    index = torch.empty((B, A, K), dtype=i32, device=dev)
    slot_state = torch.empty((B, A, K), dtype=i32, device=dev)
    nat.call('tds_stop_lines_f32', dev, _c(agent_xy.detach()), _c(agent_sc.detach()), _u8(agent_present), _c(lines.detach()), _c(line_sc.detach()), _u8(mask),
             _c(state, torch.int64), None if time_to_change is None else _c(time_to_change), features, index, slot_state, B, A, N, K, float(max_distance),
             int(bool(ahead_only)), float('-inf') if min_cos is None else float(min_cos))
    return features, index, slot_state


def _aligned(t):
    """t, or a copy of it where its data does not start at a multiple of 16 bytes (a contiguous view at an odd storage offset): the backward kernels
    read a slot's incoming gradients as 16-byte loads"""
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _StopLinesGrad(torch.autograd.Function):
    """K7's stop-line observations as an autograd node: forward = stop_lines, backward = tds_stop_lines_bwd_f32 (csrc/stop_lines_bwd.hip), one launch"""

    @staticmethod
    def forward(ctx, agent_xy, agent_sc, agent_present, lines, line_sc, mask, state, time_to_change, k, max_distance, ahead_only, min_cos):
        features, index, slot_state = stop_lines(agent_xy, agent_sc, agent_present, lines, line_sc, mask, state, time_to_change, k, max_distance,
                                                 ahead_only=ahead_only, min_cos=min_cos)
        ctx.mark_non_differentiable(index, slot_state)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(agent_xy, agent_sc, index, lines, line_sc)
        return features, index, slot_state

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_features, _g_index, _g_state):
        if g_features is None or not any(ctx.needs_input_grad[:2]):
            return (None,) * 12
        agent_xy, agent_sc, index, lines, line_sc = ctx.saved_tensors
        B, A, K = index.shape
        dev = index.device
        g_xy = torch.empty((B, A, 2), dtype=f32, device=dev)
        g_sc = torch.empty((B, A, 2), dtype=f32, device=dev)
        nat.call('tds_stop_lines_bwd_f32', dev, _c(agent_xy.detach()), _c(agent_sc.detach()), _c(lines.detach()), _c(line_sc.detach()), index,
                 _aligned(_c(g_features)), g_xy, g_sc, B, A, lines.shape[1], K)
        need = ctx.needs_input_grad
        return (g_xy.to(agent_xy.dtype) if need[0] else None, g_sc.to(agent_sc.dtype) if need[1] else None) + (None,) * 10


def stop_lines_grad(agent_xy, agent_sc, agent_present, lines, line_sc, mask, state, time_to_change, k, max_distance, ahead_only=True, min_cos=None):
    """`stop_lines`, differentiable (include/tdship.h "K7b"): the same launch and the same bits; `features` carries the graph to
    `agent_xy` and to `agent_sc` = [sin psi, cos psi] of the observing agent -- the lines are constants, even where they require grad --, `index`
    and `state` never do.  The backward is ONE launch (tds_stop_lines_bwd_f32).  Which line is in a slot and the order of the slots, the
    `max_distance` cut, `ahead_only`, `min_cos` and `mask` are constants; `time_to_change`, length and width send no gradient anywhere.  An empty
    slot contributes exactly zero whatever its incoming gradient holds; an agent exactly on a line's centre gets no NaN from `distance`.  No
    double backward."""
    return _StopLinesGrad.apply(agent_xy, agent_sc, agent_present, lines, line_sc, mask, state, time_to_change, k, max_distance, ahead_only, min_cos)


# ---------------------------------------------------------------------------------------------------------------
# K8 lane observations (csrc/lane_obs.hip)
# ---------------------------------------------------------------------------------------------------------------
def check_lanes_args(k, n_points, spacing, max_distance):
    """the argument rules of tds_lane_observations_multi, on the host: raised before anything is computed or launched"""
    _check_k('lanes', k, nat.LANE_OBS_MAX_K)
    if int(n_points) != n_points or int(n_points) < 1 or int(n_points) > nat.LANE_OBS_MAX_POINTS:
        raise ValueError(f'lanes: n_points must be 1 .. {nat.LANE_OBS_MAX_POINTS} (got {n_points})')
    if not 0.0 < float(spacing) < float('inf'):         # (NaN fails the comparison)
        raise ValueError(f'lanes: spacing must be finite and positive (got {spacing})')
    _check_reach('lanes', 'max_distance', max_distance)


def empty_lane_observations(B, A, k, n_points, device):
    """the outputs of `lane_observations` with every slot empty, built with torch: what a batch without any lane map gets"""
    return (torch.zeros((B, A, k, 8), dtype=f32, device=device), torch.zeros((B, A, k, n_points, 2), dtype=f32, device=device),
            torch.zeros((B, A, k), dtype=i32, device=device), torch.full((B, A, k), -1, dtype=i32, device=device))


def lane_observations(lane_set, agent_xy, agent_sc, present, k, n_points, spacing, max_distance):
    """The k nearest lanelets of every exposed agent (tds_lane_observations_multi, include/tdship.h "K8"): lane_set a LaneTableSet (its
    scene_map, when there is one, has B entries), agent_xy (B,A,2), agent_sc (B,A,2) [sin, cos], present (B,A) -> features (B,A,k,8) float32,
    points (B,A,k,n_points,2) float32, n_valid (B,A,k) int32, index (B,A,k) int32.  One launch on the current stream, no allocation besides
    the outputs, no synchronisation.  No gradient; CPU tensors raise (there is no CPU fallback)."""
    check_lanes_args(k, n_points, spacing, max_distance)
    if agent_xy.dim() != 3 or agent_xy.shape[-1] != 2:
        raise ValueError(f'lanes: agent_xy must be (B, A, 2), got {tuple(agent_xy.shape)}')
    B, A, K, P = int(agent_xy.shape[0]), int(agent_xy.shape[1]), int(k), int(n_points)
    if tuple(agent_sc.shape) != (B, A, 2) or tuple(present.shape) != (B, A):
        raise ValueError(f'lanes: agent_sc must be ({B}, {A}, 2) and present ({B}, {A}), got {tuple(agent_sc.shape)} and {tuple(present.shape)}')
    agent_xy, agent_sc, present = _c(agent_xy.detach()), _c(agent_sc.detach()), _u8(present)
    dev = agent_xy.device
    nat.dev_ptr(agent_xy, f32, 'agent_xy')                     # (a CPU tensor is refused before the lane set is looked at)
    scene_map = _scene_map(lane_set, B, 'lane_observations')
    features = torch.empty((B, A, K, 8), dtype=f32, device=dev)
    points = torch.empty((B, A, K, P, 2), dtype=f32, device=dev)
    n_valid = torch.empty((B, A, K), dtype=i32, device=dev)
    index = torch.empty((B, A, K), dtype=i32, device=dev)
    nat.call('tds_lane_observations_multi', dev, lane_set.handle, scene_map, agent_xy, agent_sc, present, features, points, n_valid, index, B, A, K, P,
             float(spacing), float(max_distance))
    return features, points, n_valid, index


class _LaneObservationsGrad(torch.autograd.Function):
    """K8 as an autograd node: forward = lane_observations, backward = tds_lane_observations_bwd_multi (csrc/lane_obs_bwd.hip), one launch"""

    @staticmethod
    def forward(ctx, agent_xy, agent_sc, lane_set, present, k, n_points, spacing, max_distance):
        features, points, n_valid, index = lane_observations(lane_set, agent_xy, agent_sc, present, k, n_points, spacing, max_distance)
        ctx.mark_non_differentiable(n_valid, index)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(agent_xy, agent_sc, index)
        # holding the set keeps the device tables alive until the backward
        ctx.lane_set, ctx.scene_map = lane_set, _scene_map(lane_set, index.shape[0], 'lane_observations')
        ctx.n_points, ctx.spacing = int(n_points), float(spacing)
        return features, points, n_valid, index

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_features, g_points, _g_n_valid, _g_index):
        if (g_features is None and g_points is None) or not any(ctx.needs_input_grad[:2]):
            return (None,) * 8
        agent_xy, agent_sc, index = ctx.saved_tensors
        B, A, K = index.shape
        dev = index.device
        g_xy = torch.empty((B, A, 2), dtype=f32, device=dev)
        g_sc = torch.empty((B, A, 2), dtype=f32, device=dev)
        nat.call('tds_lane_observations_bwd_multi', dev, ctx.lane_set.handle, ctx.scene_map, _c(agent_xy.detach()), _c(agent_sc.detach()), index,
                 None if g_features is None else _aligned(_c(g_features)), None if g_points is None else _aligned(_c(g_points)), g_xy, g_sc, B, A, K,
                 ctx.n_points, ctx.spacing)
        need = ctx.needs_input_grad
        return (g_xy.to(agent_xy.dtype) if need[0] else None, g_sc.to(agent_sc.dtype) if need[1] else None) + (None,) * 6


def lane_observations_grad(lane_set, agent_xy, agent_sc, present, k, n_points, spacing, max_distance):
    """`lane_observations`, differentiable (include/tdship.h "K8b"): the same launch and the same bits; `features` and `points`
    carry the graph to `agent_xy` and to `agent_sc` = [sin psi, cos psi] of the observing agent -- the map is constant --, `n_valid` and `index`
    never do.  The backward is ONE launch (tds_lane_observations_bwd_multi).  Which lanelet is in a slot and the order of the slots, the
    `max_distance` cut, the foot's segment, whether the foot was clamped to a segment's end and, for every point, its validity and the segment it
    lies on are constants.  An empty slot and an invalid point contribute exactly zero whatever their incoming gradient holds.  No double
    backward."""
    return _LaneObservationsGrad.apply(agent_xy, agent_sc, lane_set, present, k, n_points, spacing, max_distance)


# ---------------------------------------------------------------------------------------------------------------
# K3 rasteriser
# ---------------------------------------------------------------------------------------------------------------
#: scratch for the binned fast path of K3, one per (device, stream, cameras, resolution): two renders of one shape on different streams
#: (or threads) of a device never share it.  Never carries state between calls; the least recently used entries are dropped.
_workspaces = collections.OrderedDict()
_WORKSPACES_MAX = 8
use_workspace = True
use_bitplanes = True      # test hook: False forces the packed-key kernels
use_index_slices = True   # test hook: False makes the raster backward read the forward image (the path of the packed-key kernels)


def _raster_workspace(dev, n_img, res, out_mode=None, n_keys=-1):
    """n_keys: distinct keys of the launch (map + actors) when the caller knows them (-1: not known) -- with at most 15 the bit-plane kernels
    run, which above 160 x 160 (float32) / 216 x 216 (uint8) need nothing but their 64 bytes of work queues (128 bytes instead of 2.1 GB at
    B x A = 65 536 cameras of 256 x 256)"""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    n_keys = int(n_keys) if (out_mode is not None and 0 <= n_keys <= 15) else -1
    key = (idx, torch.cuda.current_stream(dev).cuda_stream, threading.get_ident(), n_img, res, out_mode if n_keys >= 0 else None, n_keys >= 0)
    ws = _workspaces.get(key)
    if ws is None:
        n = ctypes.c_int64(0)
        if n_keys >= 0:
            nat.call('tds_raster_scene_workspace_bytes_for', dev, n_img, res, out_mode, n_keys, ctypes.byref(n))
        else:
            nat.call('tds_raster_scene_workspace_bytes', dev, n_img, res, ctypes.byref(n))
        ws = torch.empty(max(int(n.value), 0), dtype=torch.uint8, device=dev) if n.value > 0 else False
        _workspaces[key] = ws
        while len(_workspaces) > _WORKSPACES_MAX:
            _workspaces.popitem(last=False)            # the tensor is freed stream-ordered by the caching allocator
    else:
        _workspaces.move_to_end(key)
    return ws if ws is not False else None


#: The persistent bit-plane launch computes each camera's scan set-up (trim polygon, grid window, grid rows) once, in a small kernel in front of
#: it, when it is given a table for the records (include/tdship.h, tds_raster_aux_t::camera_prep).  The table is scratch like the workspace -- one
#: per (device, stream, thread, shape of the launch), its size asked for on a cache miss only, the least recently used dropped, nothing carried between calls -- but not part of it.  False: every workgroup
#: computes its camera's set-up itself, as before; the pixels are the same either way (tests/test_gpu_camera_prep.py).
use_camera_prep = True
#: the persistent bit-plane launches paint small map faces (inside the image, at most seven rows) on the lane that scanned them
#: (TDS_RASTER_NO_SMALL_FACES of include/tdship.h switches it off per call); the pixels are the same with it switched off
use_small_faces = True
#: ... and for differentiable calls too.  Off by default: the launch that also stores the index slices writes every line and is bound by that
#: stream, so the instructions saved buy nothing and the records' loads cost (config 5's forward launch at B = 256: 1.85 -> 1.87 - 1.89 ms with the
#: table, three alternating runs each: profiles/camera_prep_timing.json); the native path takes the table all the same and is tested.
use_camera_prep_with_slices = False
_camera_preps = collections.OrderedDict()
#: The persistent bit-plane launch of a loop in `Simulator.overlap_infractions = 'reserved'` mode runs on a stream that is kept off four CUs per XCD, for
#: the metric kernels; once those have ended (about 1.3 of the launch's 5 ms) the 32 CUs would stand idle while the launch -- bound by instruction issue
#: since it skips the background lines -- is short of SIMDs.  With this switch on, raster_scene hands the metric stream down as the launch's helper
#: stream (include/tdship.h, tds_raster_aux_helper_t): the same kernel is enqueued there a second time, its 96 workgroups start when the metrics end
#: and take items from the launch's queues.  Same pixels (tests/test_gpu_helper_cus.py); not for differentiable calls, masks, the split form, or
#: under stream capture -- the native rule is plan_raster_scene's (csrc/tds_raster_plan.h, helper_grid).
use_helper_cus = True
#: workgroups of the helper enqueue of the last raster_scene call of this process (0: the call made its one launch)
last_helper_workgroups = 0


def _camera_prep_table(dev, n_img, res, out_mode, n_keys):
    """the table of prepared scan set-ups for a launch of this shape, or None where no launch of that shape takes one"""
    if not 0 < n_keys <= 15:                  # not known, or more than the bit-plane kernels take: packed keys, no table
        return None
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (idx, torch.cuda.current_stream(dev).cuda_stream, threading.get_ident(), n_img, res, out_mode, int(n_keys))
    tab = _camera_preps.get(key)
    if tab is None:                           # the size is asked for on a miss only, as the workspace's is (False: this shape takes no table)
        n = ctypes.c_int64(0)
        nat.call('tds_raster_camera_prep_bytes', dev, n_img, res, out_mode, n_keys, ctypes.byref(n))
        tab = _camera_preps[key] = torch.empty(int(n.value), dtype=torch.uint8, device=dev) if n.value > 0 else False
        while len(_camera_preps) > _WORKSPACES_MAX:
            _camera_preps.popitem(last=False)          # the tensor is freed stream-ordered by the caching allocator
    else:
        _camera_preps.move_to_end(key)
    return tab if tab is not False else None


# ---- where the images live --------------------------------------------------------------------------------------------------------
#: The raster launch is bound by the HBM write stream, and what that stream reaches depends on the PHYSICAL pages under the image: about one
#: large hipMalloc in three is served at 7/8 of the rate for as long as it lives, a buffer whose pages are spread out hardly ever is (one of 100 probed in round 4, in the 15/16 class; csrc/alloc.hip,
#: DESIGN_HISTORY.md section 4).  So images of SPREAD_MIN bytes and more are not taken from torch's default pool but from a torch memory pool whose
#: blocks the library builds (tds_torch_alloc / tds_torch_free behind torch.cuda.memory.CUDAPluggableAllocator): the reference-shaped call
#: `render_egocentric()` -- a fresh tensor per call, rendering/cv2.py:52 -- gets such a block, cached and stream-ordered by torch's
#: allocator like any other.  False: plain torch.empty (tests, tools/alloc experiments).
use_image_pool = True
SPREAD_MIN = 256 << 20
_image_pools = {}            # device index -> torch.cuda.MemPool
_pool_allocators = []        # the pluggable allocators behind them: they must outlive every pool, so they live as long as the process


def image_pool(device):
    """The torch memory pool of `device` whose blocks have spread-out physical pages (one per device, created on first use)."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    pool = _image_pools.get(idx)
    if pool is None:
        nat.lib()                                         # fails loudly when the library is missing
        if not _pool_allocators:
            _pool_allocators.append(torch.cuda.memory.CUDAPluggableAllocator(nat.LIB_PATH, 'tds_torch_alloc', 'tds_torch_free'))
            atexit.register(release_image_pool)           # the pools go before the interpreter takes the allocator apart
        pool = _image_pools[idx] = torch.cuda.MemPool(_pool_allocators[0].allocator())
    return pool


def release_image_pool(device=None) -> None:
    """Drop the image pool(s): their cached blocks go back to the driver once the tensors in them are gone."""
    def _index(d):
        d = torch.device(d)
        return d.index if d.index is not None else torch.cuda.current_device()
    for idx in list(_image_pools) if device is None else [_index(device)]:
        pool = _image_pools.pop(idx, None)
        del pool                                          # the pool dies here, while its allocator is alive


def empty_image(shape, dtype, device) -> torch.Tensor:
    """torch.empty for a rendered image: from the image pool when it is large enough for the placement to matter"""
    n = 1
    for d in shape:
        n *= int(d)
    nbytes = n * torch.empty((), dtype=dtype).element_size()
    device = torch.device(device)
    if not use_image_pool or nbytes < SPREAD_MIN or device.type != 'cuda' or torch.cuda.is_current_stream_capturing():
        return torch.empty(shape, dtype=dtype, device=device)
    with torch.cuda.use_mem_pool(image_pool(device), device=device):
        return torch.empty(shape, dtype=dtype, device=device)


class _OwnedBuffer:
    """a tds_buffer (csrc/alloc.hip) exposed through __cuda_array_interface__: torch.as_tensor(...) keeps it alive, the buffer goes back
    to the driver when the last tensor over it is gone"""

    def __init__(self, shape, dtype, device, dense=False):
        self.device = torch.device(device)
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        n = 1
        for d in shape:
            n *= int(d)
        self.handle = ctypes.c_void_p()
        nat.check(nat.lib().tds_buffer_create(max(n * torch.empty((), dtype=dtype).element_size(), 1), idx, nat.BUFFER_DENSE if dense else 0,
                                              ctypes.byref(self.handle)), 'tds_buffer_create')
        self._lib = nat.lib()
        typestr = {torch.float32: '<f4', torch.uint8: '|u1', torch.int32: '<i4'}[dtype]
        self.__cuda_array_interface__ = dict(shape=tuple(int(d) for d in shape), typestr=typestr, data=(int(self._lib.tds_buffer_ptr(self.handle)), False),
                                             version=2, strides=None)

    def __del__(self, _finalizing=sys.is_finalizing):      # (bound at definition: module globals are gone when the interpreter shuts down)
        h, self.handle = getattr(self, 'handle', None), None
        if h and not _finalizing():                        # at interpreter shutdown the driver takes the memory back itself
            _owned_buffers.pop(self.__cuda_array_interface__['data'][0], None)      # with it the coverage record: the address may be handed out again
            try:
                torch.cuda.synchronize(self.device)            # nothing in flight may still write to pages that are about to be unmapped
            except Exception:                                  # noqa: BLE001 -- interpreter shutdown
                pass
            self._lib.tds_buffer_destroy(h)


def owned_image(shape, dtype=torch.float32, device="cuda", dense=False) -> torch.Tensor:
    """A caller-owned image buffer with spread-out physical pages that does NOT go through torch's caching allocator (long-lived output
    rings: rendering.allocate_image_ring); freed when the tensor and all its views are gone."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    buf = _OwnedBuffer(shape, dtype, device, dense=dense)
    t = torch.as_tensor(buf, device=device)
    _owned_buffers[t.data_ptr()] = dict(nbytes=t.numel() * t.element_size(), shape=tuple(t.shape), dtype=dtype, record=None)
    return t


# ---- which lines of an owned image hold something ---------------------------------------------------------------------------------------
#: A loop renders into a ring of owned buffers: what a buffer holds when it is rendered into is the same cameras' image of `count` steps ago,
#: and about half of its 128-byte lines held only background then and hold only background now.  The fused bit-plane kernel keeps a COVERAGE
#: RECORD per buffer (include/tdship.h, tds_raster_aux_t::coverage: one bit per line) and leaves those lines alone (53 % of the lines
#: in tests/test_gpu_write_skipping.py; the headline launch 6.90 -> 6.13 ms, profiles/write_skip_timing.json).  Only the buffers of `owned_image` are tracked (the library sees them die); the image pool and arbitrary caller tensors
#: are written in full as ever.  What the host knows about a buffer's contents is torch's version counter of the tensor it was handed:
#:     WRITES THAT DO NOT BUMP IT ARE NOT SEEN -- raw-pointer writes of other libraries, writes through `.data`, a replayed graph that
#:     writes into the buffer.  A caller that does any of these switches skipping off (`use_write_skipping = False`,
#:     HipRendererConfig.write_skipping) or calls `forget_coverage(buf)` after the write.
#: False: every line is stored (the record is still kept up to date, so that switching back on needs no full write).
use_write_skipping = True
_owned_buffers = {}          # address of an _OwnedBuffer -> dict(nbytes, shape, dtype, record); gone with the buffer
_NO_VERSION = object()


def write_skip_decision(record, whole_buffer, res, n_img, version, capturing, enabled):
    """What a float32 render into an owned buffer does with the buffer's coverage record.  Plain values in, so that a CPU test can drive it:
    `record` None or dict(res, n_img, version (the tensor's version counter after the last render), valid); `whole_buffer`: `out` is the buffer as it
    was allocated (same address, shape and dtype, contiguous); `version`: out._version now, _NO_VERSION when it cannot be read (inference
    tensors); `capturing`: the stream is being captured; `enabled`: the two switches.  ->
      'untracked'  no record is passed and the one there is is dropped: every line is stored.  Part of the buffer, a resolution that is no multiple
                   of 32, no version counter -- and stream capture: a graph must not hold the address of a record that dies with its buffer.
      'rewrite'    TDS_RASTER_REWRITE_ALL: every line is stored and the coverage recorded.  No (valid) record, another resolution or camera
                   count, the tensor was written to since the last render, or skipping is switched off.
      'skip'       the lines that were background and stay background are left alone."""
    if not whole_buffer or res % 32 != 0 or version is _NO_VERSION or capturing:
        return 'untracked'
    if record is None or not record.get('valid') or (record['res'], record['n_img']) != (res, n_img) or record['version'] != version or not enabled:
        return 'rewrite'
    return 'skip'


def _owned_overlapping(t):
    lo = t.data_ptr()
    hi = lo + max(t.numel() * t.element_size(), 1)
    return [ent for ptr, ent in _owned_buffers.items() if ptr < hi and lo < ptr + ent['nbytes']]


def forget_coverage(buf) -> None:
    """Drop what the library believes an owned buffer holds: the next render into it (or into the buffer any part of which `buf` views) stores
    every line.  For writers the version counter does not show (see use_write_skipping)."""
    if isinstance(buf, torch.Tensor) and buf.is_cuda and _owned_buffers:
        for ent in _owned_overlapping(buf):
            if ent['record'] is not None:
                ent['record']['valid'] = False             # (the allocation stays: nothing is freed, nothing waits, between two renders)


def _coverage_aux(out, res, n_img, enabled):
    """-> (entry of the owned buffer `out` is, decision, record) for a float32 colour render into the caller's `out`; (None, 'untracked', None) when
    `out` is no owned buffer or only touches one (whose record is dropped: its lines are about to change under it)"""
    ent = _owned_buffers.get(out.data_ptr())
    whole = ent is not None and ent['shape'] == tuple(out.shape) and ent['dtype'] == out.dtype and out.is_contiguous()
    try:
        version = out._version
    except Exception:                                          # noqa: BLE001 -- inference tensors have no version counter
        version = _NO_VERSION
    decision = write_skip_decision(ent['record'] if whole else None, whole, res, n_img, version, torch.cuda.is_current_stream_capturing(), enabled)
    if decision == 'untracked':
        forget_coverage(out)
        return None, decision, None
    rec = ent['record']
    if rec is None or (rec['res'], rec['n_img']) != (res, n_img):
        nbytes = ctypes.c_int64(0)
        nat.call('tds_raster_coverage_bytes', out.device, n_img, int(res), ctypes.byref(nbytes))
        # the library's memory like the buffer itself, not torch's: it lives as long as the buffer, whatever stream renders into it
        cov = torch.as_tensor(_OwnedBuffer((nbytes.value // 4,), i32, out.device), device=out.device)
        rec = dict(cov=cov, res=res, n_img=n_img, version=None, valid=False)
    ent['record'] = None                                       # until the call has come back and said that it maintained the record
    return ent, decision, rec


# ---- streams confined to a part of the CUs ---------------------------------------------------------------------------------------------
_reserved_streams = {}       # (device index, CUs per XCD) -> (raster stream, metric stream, handles kept alive)


def check_reserved_layout(raster_places, metric_places, per_xcd: int, cus: int):
    """Is what the two masked streams REALLY run on the layout `overlap_infractions = 'reserved'` relies on?  `*_places`: the distinct
    XCC_ID << 16 | SE/SH/CU words that tds_stream_places reported for the raster stream and for the metric stream.  Wanted: the metric
    stream on exactly `per_xcd` CUs of EVERY XCD, the raster stream on all the others, no CU in both, at least 64 CUs in all (a CPX partition
    of 32 CUs has nothing to give away).  -> (ok, reason).  Pure host logic: tests/test_host_logic.py feeds it good, shifted and small layouts."""
    raster, metric = set(int(p) for p in raster_places), set(int(p) for p in metric_places)
    if cus < 64:
        return False, f'the device reports {cus} CUs: too few to keep {per_xcd} per XCD free of the raster launch'
    if not raster or not metric:
        return False, 'a masked stream ran nowhere'
    if raster & metric:
        return False, f'{len(raster & metric)} CUs serve both streams: the mask bits do not mean what they mean on an MI355X in SPX mode'
    xcds = sorted({p >> 16 for p in raster | metric})
    per = {x: sum(1 for p in metric if p >> 16 == x) for x in xcds}
    if any(n != per_xcd for n in per.values()):
        return False, f'the metric stream has {per} CUs per XCD instead of {per_xcd} on each'
    if len(raster) + len(metric) != cus:
        return False, f'the two streams cover {len(raster) + len(metric)} of {cus} CUs'
    return True, 'ok'


def stream_places(stream, n: int = 8192):
    """the distinct places (XCC_ID << 16 | SE/SH/CU) the kernels of a torch stream run on (tds_stream_places; synchronises)"""
    dev = stream.device
    out = torch.full((n,), -1, dtype=i32, device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    nat.call('tds_stream_places', dev, stream, out, n)      # (with `dev` current)
    stream.synchronize()
    return sorted(set(out.cpu().tolist()))


def reserved_streams(device, per_xcd: int = 4):
    """(raster_stream, metric_stream) of `device`: two torch.cuda.ExternalStream over tds_stream_create -- the first may use every CU but
    `per_xcd` per XCD, the second ONLY those (mask bit i is CU i / 8 of XCD i % 8 on MI355X, tools/cu_mask_probe.hip).  The persistent raster
    launch holds every CU it may use until its last image is out; kept off 32 of the 256 it loses nothing where it is bound by the write stream
    (every line stored), and where it is bound by instruction issue (background lines skipped) it gets the 32 back as soon as the metrics have
    ended (`use_helper_cus`); the metric kernels have somewhere to run beside it (Simulator.overlap_infractions = 'reserved').  Created once per device; the
    layout is VERIFIED on the device when the streams are made (reserved_layout_ok)."""
    ent = _reserved_entry(device, per_xcd)
    if ent[0] is None:
        raise RuntimeError(f"no CU-masked streams on this device: {ent[3][1]}")
    return ent[0], ent[1]


def reserved_layout_ok(device, per_xcd: int = 4):
    """(ok, reason): can `overlap_infractions = 'reserved'` be used on this device?  The mask layout is an observation of one part in one
    partition mode; here a probe kernel on each of the two streams reports where it really ran (tds_stream_places) and check_reserved_layout
    judges it.  Never raises: a device too small for the masks answers (False, why)."""
    return _reserved_entry(device, per_xcd)[3]


def _reserved_entry(device, per_xcd):
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    ent = _reserved_streams.get((idx, per_xcd))
    if ent is not None and ent[0] is not None and ent[3][1].startswith('not verified') and not torch.cuda.is_current_stream_capturing():
        # the streams were made under stream capture, where no probe can run: judged now, at the first call outside capture
        try:
            with torch.cuda.device(idx):
                cus = ctypes.c_int(0)
                nat.check(nat.lib().tds_device_cu_count(idx, ctypes.byref(cus)), 'tds_device_cu_count')
                verdict = check_reserved_layout(stream_places(ent[0]), stream_places(ent[1]), per_xcd, cus.value)
        except Exception as exc:                                     # noqa: BLE001 -- 'never raises': the mode falls back with one warning
            verdict = (False, f'the probe of the CU-masked streams failed: {exc}')
        ent = _reserved_streams[(idx, per_xcd)] = (ent[0], ent[1], ent[2], verdict)
    if ent is None:
        try:
            with torch.cuda.device(idx):
                ent = _make_reserved_entry(idx, per_xcd)
        except Exception as exc:                                     # noqa: BLE001 -- reserved_layout_ok / Simulator._reserved_usable promise not to raise
            ent = (None, None, [], (False, f'creating or probing the CU-masked streams failed: {exc}'))
        _reserved_streams[(idx, per_xcd)] = ent
    return ent


def _make_reserved_entry(idx, per_xcd):
    """(raster stream, metric stream, handles, (ok, reason)) of device `idx` (current); (None, None, [], (False, why)) on a device too small"""
    L = nat.lib()
    cus = ctypes.c_int(0)
    nat.check(L.tds_device_cu_count(idx, ctypes.byref(cus)), 'tds_device_cu_count')
    n_words = (cus.value + 31) // 32
    reserved = [0] * n_words
    for bit in range(min(8 * per_xcd, cus.value)):
        reserved[bit // 32] |= 1 << (bit % 32)
    every = [0] * n_words
    for bit in range(cus.value):
        every[bit // 32] |= 1 << (bit % 32)
    rest = [e & ~r for e, r in zip(every, reserved)]
    if cus.value < 64 or not any(rest) or not any(reserved):
        return None, None, [], (False, f'the device reports {cus.value} CUs: too few to keep {per_xcd} per XCD free of the raster launch')
    handles = []
    for mask in (rest, reserved):
        arr = (ctypes.c_uint32 * n_words)(*mask)
        h = ctypes.c_void_p()
        nat.check(L.tds_stream_create(idx, ctypes.cast(arr, ctypes.c_void_p), n_words, ctypes.byref(h)), 'tds_stream_create')
        handles.append(h)
    rs = torch.cuda.ExternalStream(handles[0].value, device=torch.device('cuda', idx))
    ms = torch.cuda.ExternalStream(handles[1].value, device=torch.device('cuda', idx))
    if torch.cuda.is_current_stream_capturing():
        verdict = (True, 'not verified: created under stream capture')          # judged at the first call outside capture (_reserved_entry)
    else:
        verdict = check_reserved_layout(stream_places(rs), stream_places(ms), per_xcd, cus.value)
    return rs, ms, handles, verdict


#: set to a list to have raster_scene append (start, end) torch.cuda.Event pairs recorded around every kernel launch
raster_events = None
#: the same for the launches of the raster backward kernel
raster_bwd_events = None
#: calls of raster_scene so far in this process (bench.py reports which of them its timed region was, so that a kernel trace of the run can
#: be cut to exactly those launches: tools/make_profiles.py)
raster_calls = 0


def _scene_call(fn, smap, state, agent_sc, tmpl, actor_key, mask, cam_xy, cam_sc, extra_tri, extra_key, fov, res, mode, out, out_tail, out_dtype):
    """What raster_scene and raster_scene_masks prepare alike: the sizes, the dense inputs, the per-camera triangles, the map set's scene count and
    `out` (checked, or allocated: B x Nc x out_tail of out_dtype).  -> (B, Nc, N, K, actor_key, extra_key, out, call): the dense keys and
    call(middle, tail), the C call of entry point `fn` (`fn`_multi for a StaticMapSet) with `middle` (workspace, key table ...) between the
    arguments both entry points take first and the per-camera triangles, `tail` after them.  `call` holds the dense inputs: their pointers
    are taken when it runs."""
    B, Nc = cam_xy.shape[:2]
    N = state.shape[1]
    dev = cam_xy.device
    cam_xy, cam_sc = _c(cam_xy), _c(cam_sc)
    if N > 0:
        state, agent_sc, tmpl = _c(state), _c(agent_sc), _c(tmpl)
        actor_key = _c(actor_key, i32)
        assert tuple(actor_key.shape) in ((B, N, 2), (B, Nc, N, 2)), 'actor_key must be (B,N,2) or (B,Nc,N,2)'
        mask = _u8(mask)
    shape = (B, Nc) + tuple(out_tail)
    if out is None:
        out = empty_image(shape, out_dtype, dev)
    else:
        # a real error, not an assert (python -O strips those), on anything the kernel's 16-byte non-temporal stores cannot take
        if tuple(out.shape) != shape or out.dtype != out_dtype or not out.is_contiguous():
            raise RuntimeError(f'`out` must be a contiguous {out_dtype} tensor of shape {shape}, got {out.dtype} {tuple(out.shape)}'
                               f'{"" if out.is_contiguous() else " (not contiguous)"}')
        if out.device != dev:
            raise RuntimeError(f'`out` is on {out.device}, the cameras on {dev}')
        if out.data_ptr() % 16 != 0:
            raise RuntimeError('`out` must be 16-byte aligned (a view with an odd storage offset is not)')
    K = 0
    if extra_tri is not None and extra_tri.shape[2] > 0:
        K = extra_tri.shape[2]
        assert tuple(extra_tri.shape) == (B, Nc, K, 3, 2) and tuple(extra_key.shape) == (B, Nc, K), 'extra_tri must be (B,Nc,K,3,2), extra_key (B,Nc,K)'
        extra_tri, extra_key = _c(extra_tri), _c(extra_key, i32)
    if isinstance(smap, StaticMapSet) and smap.scene_map.shape[0] != B:
        raise RuntimeError(f'the StaticMapSet is for {smap.scene_map.shape[0]} scenes, the cameras for {B}')
    actors = (state, agent_sc, tmpl, actor_key, mask) if N > 0 else (None,) * 5
    extra = (extra_tri, extra_key) if K > 0 else (None, None)

    def call(middle, tail):
        nat.call(*_map_head(fn, '', smap, dev), *actors, cam_xy, cam_sc, B, Nc, N, float(2.0 / fov), int(res), mode, nat.dev_ptr(out, out_dtype, 'out'),
                 *middle, *extra, K, *tail)
    return B, Nc, N, K, actor_key, extra_key, out, call


def raster_scene(smap, state, agent_sc, tmpl, actor_key, mask, cam_xy, cam_sc, fov, res, out_dtype=torch.float32, out=None, key_table=None,
                 extra_tri=None, extra_key=None, index_slices=False, trim=True, write_skipping=True, camera_prep=True, small_faces=True,
                 helper_stream=None):
    """Fused Simulator.render: state (B,N,4), agent_sc (B,N,2), tmpl (B,N,7,2), actor_key (B,N,2) int32 bit patterns -- or (B,Nc,N,2)
    when every camera sees its own colours (custom_agent_colors) --, mask (B,Nc,N) bool/uint8, cam_xy / cam_sc (B,Nc,2)
    -> (B,Nc,3,res,res) float32 [0,255] or uint8.  extra_tri (B,Nc,K,3,2) world-space triangles with keys extra_key (B,Nc,K) int32
    (0 = none) are drawn per camera (waypoint discs); their keys belong into `key_table` too.
    index_slices=True: returns (image, slices, keys) -- the per-pixel key index as bit-slices (int32 tensor, layout in include/tdship.h)
    and the ascending key table of the launch, what the backward pass reads instead of the image; (image, None, None) when the call
    cannot be served by the bit-plane kernel.
    `out` an `owned_image` buffer (float32): the lines that held background after the last render into it and hold background again are not
    stored a second time (see `use_write_skipping` for what the caller must not do to the buffer in between); write_skipping=False stores them.
    camera_prep=False (or `use_camera_prep`): no table of prepared scan set-ups is passed -- same pixels, the set-up is computed per workgroup.
    helper_stream (a torch stream confined to CUs the current stream is kept off, see `use_helper_cus`): the persistent launch is enqueued there a
    second time, behind whatever that stream holds; the current stream waits for it before the call returns.  `last_helper_workgroups` says
    whether the launch took it."""
    assert out_dtype in (torch.float32, torch.uint8)
    dev = cam_xy.device
    mode = nat.OUT_F32 if out_dtype == torch.float32 else nat.OUT_U8
    caller_out = out
    B, Nc, N, K, actor_key, extra_key, out, call = _scene_call('tds_raster_scene', smap, state, agent_sc, tmpl, actor_key, mask, cam_xy, cam_sc,
                                                               extra_tri, extra_key, fov, res, mode, out, (3, res, res), out_dtype)
    # distinct actor keys (host side): enables the bit-plane kernel.  Callers that know them (Simulator) pass `key_table`;
    # otherwise they are read back from the device tensor (a synchronisation -- fine for tests and one-off calls)
    if key_table is None and (N > 0 or K > 0) and use_bitplanes:
        parts = ([actor_key.flatten()] if N > 0 else []) + ([extra_key.flatten()] if K > 0 else [])
        key_table = [v for v in torch.unique(torch.cat(parts)).cpu().tolist() if v != 0]
    kt = None
    if key_table is not None and use_bitplanes:
        vals = [int(v) & 0xffffffff for v in key_table]
        kt = (ctypes.c_uint32 * max(len(vals), 1))(*vals)
    n_keys = -1
    if kt is not None:
        n_keys = len(set(vals) | set(smap.face_keys())) if smap.face_keys() is not None else -1
    ws = _raster_workspace(dev, B * Nc, int(res), mode, n_keys) if use_workspace else None
    ev = None
    if raster_events is not None:          # bench.py: HIP events on the launch stream, right around the kernel
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record(torch.cuda.current_stream(dev))
    aux = slices = None
    if index_slices and kt is not None and out_dtype == torch.float32 and res % 4 == 0 and B * Nc > 0:
        nbytes = ctypes.c_int64(0)
        nat.call('tds_raster_index_slices_bytes', dev, B * Nc, int(res), ctypes.byref(nbytes))
        slices = torch.empty(nbytes.value // 4, dtype=i32, device=dev)
        aux = nat.RasterAuxHelper(index_slices=slices.data_ptr(), index_slices_bytes=nbytes.value)
    if not trim:
        aux = aux if aux is not None else nat.RasterAuxHelper()
        aux.flags = nat.RASTER_NO_TRIM
    if not (use_small_faces and small_faces):
        aux = aux if aux is not None else nat.RasterAuxHelper()
        aux.flags |= nat.RASTER_NO_SMALL_FACES
    cov_ent = cov_rec = None
    if caller_out is not None and _owned_buffers:
        if out_dtype == torch.float32 and slices is None and B * Nc > 0:
            cov_ent, decision, cov_rec = _coverage_aux(caller_out, int(res), B * Nc, use_write_skipping and write_skipping)
            if cov_rec is not None:
                aux = aux if aux is not None else nat.RasterAuxHelper()
                aux.coverage, aux.coverage_bytes = cov_rec['cov'].data_ptr(), cov_rec['cov'].numel() * 4
                if decision != 'skip':
                    aux.flags |= nat.RASTER_REWRITE_ALL
        else:
            forget_coverage(caller_out)
    prep = None
    if use_camera_prep and camera_prep and ws is not None and B * Nc > 0 and (slices is None or use_camera_prep_with_slices):
        prep = _camera_prep_table(dev, B * Nc, int(res), mode, n_keys)
    if prep is not None:
        aux = aux if aux is not None else nat.RasterAuxHelper()
        aux.camera_prep, aux.camera_prep_bytes = prep.data_ptr(), prep.numel()
        aux.flags |= nat.RASTER_HAS_CAMERA_PREP          # (the struct has the two fields)
    if use_helper_cus and helper_stream is not None and ws is not None and slices is None and B * Nc > 0:        # (stream capture: the native call checks)
        aux = aux if aux is not None else nat.RasterAuxHelper()
        aux.helper_stream = helper_stream.cuda_stream
        aux.flags |= nat.RASTER_HAS_HELPER_STREAM        # (RasterAuxHelper: the struct has the two fields)

    def launch(aux):
        call((ws, 0 if ws is None else ws.numel(), kt, 0 if kt is None else len(key_table), 1 if (N > 0 and actor_key.dim() == 4) else 0),
             (None if aux is None else ctypes.byref(aux),))

    global raster_calls, last_helper_workgroups
    raster_calls += 1
    last_helper_workgroups = 0
    try:
        launch(aux)
    except nat.TdsError as e:
        # only a documented capacity (more than 15 keys, planes too large for the bit-plane kernel: TDS_ELIMIT) sends the call to the kernels
        # that produce no slices; a bad argument (TDS_EINVAL: wrong byte count, wrong dtype ...) or a HIP failure is the caller's to see
        if aux is None or slices is None or e.code != nat.E_LIMIT:
            raise
        slices = None
        aux = None if trim else nat.RasterAux(flags=nat.RASTER_NO_TRIM)
        launch(aux)
    if cov_rec is not None:
        # a call that raised has left the buffer without a record; one that another kernel served (aux.coverage_maintained == 0: every line was stored,
        # the record not touched) keeps the allocation for the next call, marked as describing nothing
        try:
            cov_rec.update(version=caller_out._version, valid=bool(aux is not None and aux.coverage_maintained))
            cov_ent['record'] = cov_rec
        except Exception:                                      # noqa: BLE001 -- no version counter after all
            pass
    if isinstance(aux, nat.RasterAuxHelper) and aux.flags & nat.RASTER_HAS_HELPER_STREAM:
        last_helper_workgroups = int(aux.helper_workgroups)
    if ev is not None:
        ev[1].record(torch.cuda.current_stream(dev))
        raster_events.append(ev)
    if index_slices:
        if slices is None or aux is None or aux.n_keys == 0:
            return out, None, None
        return out, slices, [int(aux.keys[i]) for i in range(aux.n_keys)]
    return out


def mask_table(smap, actor_keys, key_channels):
    """The key table of a mask launch -- the distinct keys of the map (over the set) and of `actor_keys`, ascending -- and, aligned with it, the
    channel set of every key: key_channels.get(key, 0).  Raises when the map has more than 64 distinct keys (the masks need at most 15)."""
    face = smap.face_keys()
    if face is None:
        raise RuntimeError('semantic masks: the map has more than 64 distinct face keys (the bit-plane kernels take at most 15 keys)')
    table = sorted(set(int(k) & 0xffffffff for k in face) | set(int(k) & 0xffffffff for k in actor_keys))
    return table, [int(key_channels.get(k, 0)) & 0xffffffff for k in table]


@torch.no_grad()
def raster_scene_masks(smap, state, agent_sc, tmpl, actor_key, mask, cam_xy, cam_sc, fov, res, key_table, key_channels, n_channels, packed=False,
                       out=None, extra_tri=None, extra_key=None, trim=True):
    """Semantic bird's-eye masks of the scene raster_scene would draw (same arguments; actor_key (B,N,2) only): `n_channels` binary channels,
    channel c set wherever the image would paint a face whose key k has bit c in key_channels[k] (dict key -> channel set), occlusion ignored.
    key_table: the actors' (and per-camera triangles') distinct keys.  -> (B,Nc,C,res,res) torch.bool (memory order of the image: the last two
    axes are x, y), or with packed=True (B,Nc,C,ceil(res/32),res) int32 words holding bit i of pixel (32 xw + i, y) (rendering.unpack_mask_bits).
    `out`: a caller-owned contiguous tensor of that shape and dtype.  Never differentiable (no autograd graph is recorded here)."""
    B, N = cam_xy.shape[0], state.shape[1]
    if N > 0 and tuple(actor_key.shape) != (B, N, 2):
        raise RuntimeError(f'actor_key must be ({B}, {N}, 2), got {tuple(actor_key.shape)}')
    C = int(n_channels)
    if not 1 <= C <= 32:
        raise ValueError(f'semantic masks take 1 to 32 channels, got {C}')
    dev = cam_xy.device
    mode = nat.OUT_MASK_BITS if packed else nat.OUT_MASK_U8
    tail, dtype = ((C, (res + 31) // 32, res), i32) if packed else ((C, res, res), torch.bool)
    forget_coverage(out)                        # (masks rendered over an owned image buffer: its lines are no longer what the record says)
    B, Nc, _, _, _, _, out, call = _scene_call('tds_raster_scene_masks', smap, state, agent_sc, tmpl, actor_key, mask, cam_xy, cam_sc, extra_tri,
                                               extra_key, fov, res, mode, out, tail, dtype)
    actors = [int(v) & 0xffffffff for v in key_table]
    table, chans = mask_table(smap, actors, key_channels)
    kt = (ctypes.c_uint32 * max(len(actors), 1))(*actors)
    kc = (ctypes.c_uint32 * max(len(chans), 1))(*chans)
    # (more than 15 keys: the call reports TDS_ELIMIT; the workspace is sized as for 15 rather than for the packed-key kernels' lists)
    ws = _raster_workspace(dev, B * Nc, int(res), mode, min(len(table), 15))
    aux = None if trim else nat.RasterAux(flags=nat.RASTER_NO_TRIM)
    call((ws, ws.numel(), kt, len(actors)), (kc, C, None if aux is None else ctypes.byref(aux)))
    return out


class _RasterScene(torch.autograd.Function):
    """Differentiable wrapper of the fused scene rasteriser.  Forward: tds_raster_scene (CV2 pixel semantics).  Backward: the build-defined
    edge-sampling gradient with respect to actor position / heading / template vertices (sizes) and camera position / heading (DESIGN.md "K3 backward"); the
    reference's CV2 backend has none (rendering/cv2.py:27-70).  When the bit-plane kernel serves the forward it also leaves the per-pixel key
    index as bit-slices (3 % of the image), and the backward (tds_raster_scene_bwd_idx_f32) reads those and the incoming gradient next
    to colour boundaries only; otherwise the forward image is kept and tds_raster_scene_bwd_f32 streams image and gradient in full."""

    @staticmethod
    def forward(ctx, state, agent_sc, cam_xy, cam_sc, key_colors, smap, tmpl, actor_key, mask, fov, res, key_table, extra_tri, extra_key, color_keys, trim,
                ego=0):
        # ego = Nc > 0: the cameras ARE the first Nc agents (render_egocentric): positions and headings are taken from `state` / `agent_sc` here,
        # and the backward folds the cameras' gradient into the agents' -- no slice nodes in the graph, no separate gradient tensors
        ctx.ego = int(ego)
        if ctx.ego:
            cam_xy, cam_sc = state[:, :ctx.ego, :2].contiguous(), agent_sc[:, :ctx.ego].contiguous()
        out, slices, keys = raster_scene(smap, state, agent_sc, tmpl, actor_key, mask, cam_xy, cam_sc, fov, res, key_table=key_table,
                                         extra_tri=extra_tri, extra_key=extra_key, index_slices=True, trim=trim) if use_index_slices else \
            (raster_scene(smap, state, agent_sc, tmpl, actor_key, mask, cam_xy, cam_sc, fov, res, key_table=key_table, extra_tri=extra_tri,
                          extra_key=extra_key, trim=trim), None, None)
        if slices is not None:
            ctx.save_for_backward(state, agent_sc, cam_xy, cam_sc, tmpl, mask, slices)
        else:
            ctx.save_for_backward(state, agent_sc, cam_xy, cam_sc, tmpl, mask, out)
        ctx.fov, ctx.res, ctx.keys = fov, res, keys
        ctx.color_keys = None
        if key_colors is not None:
            if keys is None:
                raise RuntimeError('colour gradients need the key-index slices of the bit-plane kernel (at most 15 distinct keys, float32 output, '
                                   'resolution a multiple of 4, no per-camera colours)')
            assert len(color_keys) == key_colors.shape[0] and key_colors.shape[-1] == 3, 'key_colors is (len(color_keys), 3)'
            ctx.color_keys = [int(k) & 0xffffffff for k in color_keys]
        return out

    @staticmethod
    def backward(ctx, gout):
        state, agent_sc, cam_xy, cam_sc, tmpl, mask, kept = ctx.saved_tensors
        B, Nc = cam_xy.shape[:2]
        N = state.shape[1]
        dev = cam_xy.device
        # a gradient that is one image broadcast over the cameras (image.sum(), a fixed linear read-out ...) stays one image
        gstride = 3 * int(ctx.res) * int(ctx.res)
        if ctx.keys is not None and gout.dim() == 5 and gout.stride(0) == 0 and gout.stride(1) == 0 and B * Nc > 1:
            gout, gstride = _c(gout[0, 0]), 0
        else:
            gout = _c(gout)
        g_agent = torch.empty((B, Nc, max(N, 1), 4), dtype=f32, device=dev)
        g_cam = torch.empty((B, Nc, 4), dtype=f32, device=dev)
        m8 = _u8(mask)
        ev = None
        if raster_bwd_events is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record(torch.cuda.current_stream(dev))
        poses = ((_c(state), _c(agent_sc), _c(tmpl), m8) if N > 0 else (None,) * 4) + (_c(cam_xy), _c(cam_sc))
        g_tmpl = torch.empty((B, Nc, N, 7, 2), dtype=f32, device=dev) if (N > 0 and ctx.needs_input_grad[6]) else None      # template vertices: actor sizes
        tail = (B, Nc, N, float(2.0 / ctx.fov), int(ctx.res), g_agent, g_cam)
        g_color = None
        if ctx.keys is not None:
            kt = (ctypes.c_uint32 * 16)(*ctx.keys)
            if ctx.color_keys is not None and ctx.needs_input_grad[4]:
                g_color = torch.empty((B, Nc, 16, 4), dtype=f32, device=dev)
            nat.call('tds_raster_scene_bwd_idx_f32', dev, *poses, kept, kt, len(ctx.keys), gout, gstride, *tail, g_color, g_tmpl)
        else:
            nat.call('tds_raster_scene_bwd_f32', dev, *poses, kept, gout, *tail, g_tmpl)
        if ev is not None:
            ev[1].record(torch.cuda.current_stream(dev))
            raster_bwd_events.append(ev)
        ga = g_agent.sum(dim=1) if N > 0 else None                   # over cameras: (B, N, 4)
        g_state = g_sc = None
        if N > 0:
            if ctx.ego:
                ga[:, :ctx.ego] += g_cam                               # the camera of agent a is agent a
            g_state = torch.cat([ga[..., :2], _zeros_const(ga.shape[:-1] + (2,), dev)], dim=-1)
            g_sc = ga[..., 2:].contiguous()
        g_key_colors = None
        if g_color is not None:
            # rows of the launch's key table (index i + 1 <-> keys[i]) -> the caller's rows; a key that was not part of the launch shows nowhere
            per_key = g_color.sum(dim=(0, 1))[:, :3]                  # over cameras: (16, 3)
            pos = {k: i + 1 for i, k in enumerate(ctx.keys)}
            rows = torch.tensor([pos.get(k, -1) for k in ctx.color_keys], device=dev)
            g_key_colors = torch.where((rows >= 0)[:, None], per_key[rows.clamp(min=0)], torch.zeros((), device=dev))
        return (g_state, g_sc, None if ctx.ego else g_cam[..., :2].contiguous(), None if ctx.ego else g_cam[..., 2:].contiguous(), g_key_colors,
                None, None if g_tmpl is None else g_tmpl.sum(dim=1), None, None, None, None, None, None, None, None, None, None)


def raster_scene_diff(smap, state, agent_sc, tmpl, actor_key, mask, cam_xy, cam_sc, fov, res, key_table=None, extra_tri=None, extra_key=None,
                      key_colors=None, color_keys=None, trim=True, ego_cameras=0):
    """raster_scene with a backward pass (float32 output only; the per-camera triangles get no gradient).
    key_colors (K,3) float tensor + color_keys (K packed keys): a handle for COLOUR gradients -- row r stands for the colour the image shows
    where key color_keys[r] wins; the forward takes its pixels from the keys' own RGB bits (the caller keeps the two consistent), the
    backward returns d loss / d key_colors[r] = the sum of the incoming gradient over those pixels, all cameras (exact)."""
    if ego_cameras:
        # `ego_cameras` = Nc: the cameras are the first Nc agents of `state` / `agent_sc` (cam_xy / cam_sc are ignored)
        cam_xy = cam_sc = None
    return _RasterScene.apply(state, agent_sc, cam_xy, cam_sc, key_colors, smap, tmpl, actor_key, mask, float(fov), int(res), key_table, extra_tri,
                              extra_key, color_keys, bool(trim), int(ego_cameras))


def raster_mesh(verts, attrs, faces, cam_xy, cam_sc, levels, scale, res, out_dtype=torch.float32, trim=True):
    """Generic render_rgb_mesh: verts (n,V,3), attrs (n,V,3), faces (n,F,3) -> (n,3,res,res)"""
    n = cam_xy.shape[0]
    dev = cam_xy.device
    verts, attrs, cam_xy, cam_sc = _c(verts), _c(attrs), _c(cam_xy), _c(cam_sc)
    faces = _c(faces, i32)
    out = torch.empty((n, 3, res, res), dtype=out_dtype, device=dev)
    lv = (ctypes.c_float * max(len(levels), 1))(*[float(x) for x in levels])
    nat.call('tds_raster_mesh', dev, verts, attrs, faces, n, verts.shape[1], faces.shape[1], cam_xy, cam_sc, lv, len(levels), float(scale), int(res),
             nat.OUT_F32 if out_dtype == torch.float32 else nat.OUT_U8, nat.dev_ptr(out, out_dtype, 'out'), 0 if trim else nat.RASTER_NO_TRIM)
    return out


# ---------------------------------------------------------------------------------------------------------------
# lane tables and the wrong-way query (csrc/lanes.hip)
# ---------------------------------------------------------------------------------------------------------------
class LaneTableHandle(_Handle):
    """Device-resident lane table of one map (tds_lanes_t), built from the HOST arrays of `lanelet2.lane_table`."""
    _destroy_call = 'tds_lanes_destroy'

    def __init__(self, table, device='cuda', max_tolerance=1.0, cell_size=0.0):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('lane tables live on an MI355X; there is no CPU implementation')
        self.max_tolerance = float(max_tolerance)
        self.n_lanelets = int(len(table.flags))
        self._to_go = None                           # the distance table of routes to a destination: built by `lane_distances` when first asked for
        self._conflicts = {}                         # (clearance, step) -> the conflict table of junctions: built by `lane_conflicts`
        poly = np.ascontiguousarray(table.poly_xy, np.float64)
        cl = np.ascontiguousarray(table.cl_xyz, np.float64)
        ps, cs = np.ascontiguousarray(table.poly_start, np.int32), np.ascontiguousarray(table.cl_start, np.int32)
        fl = np.ascontiguousarray(table.flags, np.int32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        handle = ctypes.c_void_p()
        nat.call('tds_lanes_create', self.device, vp(poly), vp(ps), vp(cl), vp(cs), vp(fl), self.n_lanelets, float(cell_size),
                 self.max_tolerance, ctypes.byref(handle))
        self._h = handle
        if getattr(table, 'succ_start', None) is not None:          # the lane graph (lanelet2.lane_successors)
            ss, si = np.ascontiguousarray(table.succ_start, np.int32), np.ascontiguousarray(table.succ_items, np.int32)
            if ss.shape != (self.n_lanelets + 1,) or int(ss[-1]) != len(si):
                raise ValueError('lane table: succ_start must have one entry per lanelet plus one and end at len(succ_items)')
            nat.call('tds_lanes_set_successors', self.device, self.handle, vp(ss), vp(si))

    def info(self):
        buf = (ctypes.c_int64 * 4)()
        nat.call('tds_lanes_info', self.device, self.handle, buf)
        return dict(lanelets=buf[0], nx=buf[1], ny=buf[2], bytes=buf[3])


class LaneTableSet(_Handle):
    """The lane tables of a batch (tds_laneset_t) + which of them every scene uses (`scene_map`, (B,) int32 on the device, -1 = the
    scene has no lane map; None = every scene uses table 0)."""
    _destroy_call = 'tds_laneset_destroy'

    def __init__(self, tables, scene_map=None):
        assert len(tables) > 0
        self.tables = list(tables)                   # keeps the tables alive
        self.device = self.tables[0].device
        self.scene_map = None if scene_map is None else _c(torch.as_tensor(scene_map).to(self.device), i32)
        arr = (ctypes.c_void_p * len(self.tables))(*[t.handle for t in self.tables])
        handle = ctypes.c_void_p()
        nat.call('tds_laneset_create', self.device, arr, len(self.tables), ctypes.byref(handle))
        self._h = handle
        self._distance_tables = None
        self._conflict_tables = {}

    def distance_tables(self):
        """(n tables,) int64 on the device: the address of every table's `lane_distances`, what tds_route_to_multi reads them through.  Built
        the first time a route to a destination is asked for (allocations and one launch per table not seen before: outside any capture);
        the tensors themselves live on the table objects, which this set keeps alive."""
        if self._distance_tables is None:
            self._distance_tables = torch.tensor([lane_distances(t).data_ptr() for t in self.tables], dtype=torch.int64, device=self.device)
            torch.cuda.current_stream(self.device).synchronize()            # once: whatever stream deals routes later finds the tables complete
        return self._distance_tables

    def conflict_tables(self, clearance=2.0, step=0.5):
        """(n tables,) int64 on the device: the address of every table's `lane_conflicts(table, clearance, step)`, what
        tds_lane_give_way_multi reads them through.  Built once per (clearance, step) (allocations and one launch per table not seen before:
        outside any capture); the tensors themselves live on the table objects, which this set keeps alive."""
        key = (float(clearance), float(step))
        if key not in self._conflict_tables:
            self._conflict_tables[key] = torch.tensor([lane_conflicts(t, *key)[3].data_ptr() for t in self.tables], dtype=torch.int64, device=self.device)
            torch.cuda.current_stream(self.device).synchronize()            # once: whatever stream steps the NPCs later finds the tables complete
        return self._conflict_tables[key]


def check_lane_conflicts_args(n_lanelets, clearance, step):
    """what tds_lane_conflicts_f64 refuses, refused before any tensor is touched: TdsError with the code the entry point would return"""
    for k, x in (('clearance', clearance), ('step', step)):
        if not (0.0 < float(x) < float('inf')):
            raise nat.TdsError('lane_conflicts', nat.E_INVAL, f'{k} must be finite and greater than 0 (got {x})')
    if n_lanelets > nat.CONFLICT_MAX_LANELETS:
        raise nat.TdsError('lane_conflicts', nat.E_LIMIT, f'{n_lanelets} lanelets exceed the {nat.CONFLICT_MAX_LANELETS} whose exclusions a workgroup holds in LDS')


def lane_conflicts(table, clearance=2.0, step=0.5):
    """tds_lane_conflicts_f64 for a `LaneTableHandle`: (exit (L, L), zone_in (L,), zone_out (L,), the whole table) float64, the first three views
    of the last (include/tdship.h "Giving way at junctions").  Built once per (table, clearance, step) and kept on the table."""
    key = (float(clearance), float(step))
    L = table.n_lanelets
    check_lane_conflicts_args(L, *key)
    if key not in table._conflicts:
        whole = torch.empty((L * (L + 2),), dtype=torch.float64, device=table.device)
        nat.call('tds_lane_conflicts_f64', table.device, table.handle, whole, *key)
        table._conflicts[key] = (whole[:L * L].view(L, L), whole[L * L:L * L + L], whole[L * L + L:], whole)
    return table._conflicts[key]


def lane_distances(table):
    """tds_lane_distances_f64: the (L, L) float64 table of a `LaneTableHandle`, to_go[t][l] = distance from the start of lanelet l to the start
    of lanelet t on the lane graph (+inf: cannot be reached).  Built once per table and kept on it."""
    to_go = table._to_go
    if to_go is None:
        L = table.n_lanelets
        if L > nat.ROUTE_MAX_GRAPH:
            raise nat.TdsError('lane_distances', nat.E_LIMIT, f'{L} lanelets exceed the {nat.ROUTE_MAX_GRAPH} a destination\'s distance field holds in LDS')
        to_go = torch.empty((L, L), dtype=torch.float64, device=table.device)
        nat.call('tds_lane_distances_f64', table.device, table.handle, to_go)
        table._to_go = to_go
    return to_go


def _scene_map(lane_set, B, what):
    """the set's scene map (None: table 0 everywhere), which must be for B scenes"""
    if lane_set.scene_map is not None and lane_set.scene_map.shape[0] != B:
        raise RuntimeError(f'{what}: the lane-table set was made for {lane_set.scene_map.shape[0]} scenes, the batch has {B}')
    return lane_set.scene_map


def _scene_ids(scene_ids, B, what):
    if scene_ids is not None and tuple(scene_ids.shape) != (B,):
        raise RuntimeError(f'{what}: scene_ids must be ({B},), got {tuple(scene_ids.shape)}')
    return scene_ids


def _seed64(seed):
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def wrong_way(lane_set, state, recenter_offset, present, direction_angle_threshold, lanelet_dist_tolerance, want_dpsi=False):
    """lanelet_orientation_loss (infractions.py:232-304) [* present]: state (B,A,4) -> (B,A) float32.  No gradient from this call; `wrong_way_grad`
    is the differentiable form.  (The reference's loss does have one, to psi alone: its position passes through float() and is a constant, and so
    are the lane directions, which come from host floats, but `agent_state[2]` stays a tensor.)  With `want_dpsi` the same kernel also writes the
    derivative of the loss to psi (tds_wrong_way_grad_f32) -> (out, dloss_dpsi (B,A) float32); `out` has the same bits either way."""
    state = _c(state.detach())
    if state.dim() != 3 or state.shape[-1] != 4:
        raise RuntimeError(f'wrong_way: state must be (B,A,4), got {tuple(state.shape)}')
    B, A = state.shape[:2]
    out = torch.empty((B, A), dtype=f32, device=state.device)
    dpsi = torch.empty((B, A), dtype=f32, device=state.device) if want_dpsi else None
    if B * A == 0:
        return (out, dpsi) if want_dpsi else out
    off = None if recenter_offset is None else _c(recenter_offset.detach())
    pres = None if present is None else _u8(present)
    if want_dpsi:
        nat.call('tds_wrong_way_grad_f32', state.device, lane_set.handle, _scene_map(lane_set, B, 'wrong_way'), A, state, off, pres, out, dpsi, B * A,
                 float(direction_angle_threshold), float(lanelet_dist_tolerance))
        return out, dpsi
    nat.call('tds_wrong_way_f32', state.device, lane_set.handle, _scene_map(lane_set, B, 'wrong_way'), A, state, off, pres, out, B * A,
             float(direction_angle_threshold), float(lanelet_dist_tolerance))
    return out


class _WrongWayGrad(torch.autograd.Function):
    """the wrong-way loss as an autograd node: forward = tds_wrong_way_grad_f32, one launch; backward = g * dloss_dpsi into the psi column, in torch"""

    @staticmethod
    def forward(ctx, state, lane_set, recenter_offset, present, direction_angle_threshold, lanelet_dist_tolerance):
        out, dpsi = wrong_way(lane_set, state, recenter_offset, present, direction_angle_threshold, lanelet_dist_tolerance, want_dpsi=True)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(dpsi)
        ctx.state_dtype = state.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[0]:
            return (None,) * 6
        dpsi, = ctx.saved_tensors
        g_state = torch.zeros(tuple(dpsi.shape) + (4,), dtype=f32, device=dpsi.device)
        g_state[..., 2] = g * dpsi
        return (g_state.to(ctx.state_dtype),) + (None,) * 5


def wrong_way_grad(lane_set, state, recenter_offset, present, direction_angle_threshold, lanelet_dist_tolerance):
    """`wrong_way`, differentiable: the bits of tds_wrong_way_f32, and the result carries the graph to `state[..., 2]` alone --
    x, y and v get exactly zero, as in the reference, where the position passes through float().  d loss / d psi is -sin(delta) of the lanelet
    whose loss the minimum keeps (the first in table order of equal ones) where |delta| exceeds the threshold, else 0, and exactly 0 wherever the
    loss is forced to 0; it comes from the forward's own launch (tds_wrong_way_grad_f32), the backward is a product in torch.  Which lanelet
    attains the minimum and the threshold test are constants of differentiation.  No double backward."""
    return _WrongWayGrad.apply(state, lane_set, recenter_offset, present, direction_angle_threshold, lanelet_dist_tolerance)


def lanelet_directions(tables, scene_map, points, lanelet_dist_tolerance, max_dirs=16):
    """find_lanelet_directions for points (n,2) float64 on the device: (dirs (n,max_dirs) f64, dists (n,max_dirs) f64, count (n) i32,
    status (n) u8: bit 0 find_direction failed, bit 1 excluded tag)"""
    f64 = torch.float64
    lane_set = tables if isinstance(tables, LaneTableSet) else LaneTableSet(tables, scene_map)
    points = _c(points, f64)
    n = points.shape[0]
    dev = points.device
    dirs = torch.zeros((n, max_dirs), dtype=f64, device=dev)
    dists = torch.zeros((n, max_dirs), dtype=f64, device=dev)
    count = torch.zeros((n,), dtype=i32, device=dev)
    status = torch.zeros((n,), dtype=u8, device=dev)
    # the points are split evenly among the scenes the set was made for: the helper's size check is met by construction here
    scenes = None if lane_set.scene_map is None else lane_set.scene_map.shape[0]
    pps = 1 if scenes is None else max(1, n // max(1, scenes))
    nat.call('tds_lanelet_directions_f64', dev, lane_set.handle, _scene_map(lane_set, scenes, 'lanelet_directions'), pps, points, dirs, dists, count, status,
             max_dirs, n, float(lanelet_dist_tolerance))
    return dirs, dists, count, status


# ---------------------------------------------------------------------------------------------------------------
# on-lane scene initialisation (csrc/spawn.hip)
# ---------------------------------------------------------------------------------------------------------------
def spawn_on_lanes(lane_set, scene_ids, attributes, seed, min_speed=0.0, max_speed=10.0, gap=(1.0, 0.2), max_attempts=500, occupied=None,
                   occupied_sc=None, occupied_mask=None):
    """tds_spawn_on_lanes_f32: attributes (B,A,3) -> (state (B,A,4), sc (B,A,2), placed (B,A) bool, attempts (B,A) int32).
    lane_set: a LaneTableSet (its scene_map, when there is one, has B entries); scene_ids (B,) int64 or None = arange(B);
    occupied (B,M,5) boxes not yet inflated, occupied_sc (B,M,2) = metric_sc of the INFLATED boxes ('discs'), occupied_mask (B,M).
    One launch on the current stream, no allocation besides the outputs, no synchronisation."""
    attributes = _c(attributes)
    if attributes.dim() != 3 or attributes.shape[-1] != 3:
        raise RuntimeError(f'spawn_on_lanes: attributes must be (B,A,3), got {tuple(attributes.shape)}')
    dev = attributes.device
    B, A = attributes.shape[:2]
    nat.dev_ptr(attributes, f32, 'attributes')                 # (a CPU tensor is refused before the lane set is looked at)
    scene_map = _scene_map(lane_set, B, 'spawn_on_lanes')
    scene_ids = _scene_ids(None if scene_ids is None else scene_ids.contiguous(), B, 'spawn_on_lanes')
    M = 0
    if occupied is not None:
        occupied, occupied_sc = _c(occupied), _c(occupied_sc)
        M = occupied.shape[1]
        if tuple(occupied.shape) != (B, M, 5) or tuple(occupied_sc.shape) != (B, M, 2):
            raise RuntimeError(f'spawn_on_lanes: occupied must be ({B},M,5) with occupied_sc ({B},M,2), got {tuple(occupied.shape)}, {tuple(occupied_sc.shape)}')
        if occupied_mask is not None:
            occupied_mask = _u8(occupied_mask)
            if tuple(occupied_mask.shape) != (B, M):
                raise RuntimeError(f'spawn_on_lanes: occupied_mask must be ({B},{M}), got {tuple(occupied_mask.shape)}')
    else:
        occupied_sc = occupied_mask = None                     # (read only beside `occupied`)
    state = torch.empty((B, A, 4), dtype=f32, device=dev)
    sc = torch.empty((B, A, 2), dtype=f32, device=dev)
    placed = torch.empty((B, A), dtype=torch.bool, device=dev)
    attempts = torch.empty((B, A), dtype=i32, device=dev)
    nat.call('tds_spawn_on_lanes_f32', dev, lane_set.handle, scene_map, scene_ids, B, A, attributes, occupied, occupied_sc, occupied_mask, M, _seed64(seed),
             float(min_speed), float(max_speed), float(gap[0]), float(gap[1]), int(max_attempts), state, sc, _u8(placed), attempts)
    return state, sc, placed, attempts


# ---------------------------------------------------------------------------------------------------------------
# lane-following NPC traffic (csrc/lanes.hip: tds_lane_snap; csrc/follow.hip: tds_lane_follow_step)
# ---------------------------------------------------------------------------------------------------------------
def lane_snap(lane_set, xy, sc, tolerance=1.0, out=None):
    """tds_lane_snap_multi: xy (B,N,2) [x, y], sc (B,N,2) [sin, cos] -> (lane (B,N) int32, arc (B,N) float64, lateral (B,N) float32).
    out: the three tensors to write instead of new ones (dense, of exactly those types)."""
    xy, sc = _c(xy), _c(sc)
    if xy.dim() != 3 or xy.shape[-1] != 2 or sc.shape != xy.shape:
        raise RuntimeError(f'lane_snap: xy and sc must be (B,N,2), got {tuple(xy.shape)}, {tuple(sc.shape)}')
    B, N = xy.shape[:2]
    nat.dev_ptr(xy, f32, 'xy'), nat.dev_ptr(sc, f32, 'sc')       # (CPU tensors are refused before `out` is looked at)
    dev = xy.device
    if out is not None:
        lane, arc, lateral = out
        if any(tuple(t.shape) != (B, N) for t in out):
            raise RuntimeError(f'lane_snap: out must be three ({B},{N}) tensors, got {[tuple(t.shape) for t in out]}')
    else:
        lane = torch.empty((B, N), dtype=i32, device=dev)
        arc = torch.empty((B, N), dtype=torch.float64, device=dev)
        lateral = torch.empty((B, N), dtype=f32, device=dev)
    if B * N == 0:
        return lane, arc, lateral
    nat.call('tds_lane_snap_multi', dev, lane_set.handle, _scene_map(lane_set, B, 'lane_snap'), N, xy, sc, lane, arc, lateral, B * N, float(tolerance))
    return lane, arc, lateral


def check_lane_follow_args(n_entities, dt, horizon, lateral_margin, idm):
    """what tds_lane_follow_step refuses, refused before any tensor is touched: TdsError with the code the entry point would return"""
    if n_entities > nat.FOLLOW_MAX_ENTITIES:
        raise nat.TdsError('lane_follow_step', nat.E_LIMIT, f'{n_entities} entities exceed the {nat.FOLLOW_MAX_ENTITIES} a scene\'s LDS holds')
    values = dict(dt=dt, horizon=horizon, lateral_margin=lateral_margin, **{k: v for k, v in zip(('T', 's0', 'a', 'b', 'b_max'), idm)})
    for k, x in values.items():
        if not (0.0 <= float(x) < float('inf')):
            raise nat.TdsError('lane_follow_step', nat.E_INVAL, f'{k} must be finite and not negative (got {x})')
    if not (values['a'] > 0 and values['b'] > 0):
        raise nat.TdsError('lane_follow_step', nat.E_INVAL, 'the IDM accelerations a and b must be positive')


def lane_follow_step(lane_set, scene_ids, boxes, ent_sc, ent_speed, ent_present, self_index, npc_size, desired_speed, npc_present, lane, arc,
                     hops, state, sc, leader, seed, dt, horizon=60.0, lateral_margin=0.2, idm=(1.5, 2.0, 1.5, 2.0, 6.0), stop_at=None):
    """tds_lane_follow_step_multi (include/tdship.h; with stop_at (B,N) float64, the output of `lane_give_way`: tds_lane_follow_step_stops_multi): entities boxes (B,E,5), ent_sc (B,E,2), ent_speed (B,E), ent_present (B,E); per NPC
    self_index (B,N) int32, npc_size (B,N,2), desired_speed (B,N), npc_present (B,N); lane / arc / hops / state (B,N,4) / sc (B,N,2) / leader are
    updated IN PLACE and must be dense tensors of exactly the kernel's types.  One launch on the current stream, no allocation, no
    synchronisation.  idm = (T, s0, a, b, b_max)."""
    for name, t in (('boxes', boxes), ('ent_sc', ent_sc), ('ent_speed', ent_speed), ('ent_present', ent_present), ('npc_size', npc_size),
                    ('desired_speed', desired_speed), ('npc_present', npc_present), ('lane', lane), ('arc', arc), ('hops', hops), ('state', state),
                    ('sc', sc), ('leader', leader)):
        if not t.is_cuda:
            raise RuntimeError(f'{name}: torchdrivesim_amd kernels run on an MI355X; got a {t.device} tensor (no CPU fallback)')
    if state.dim() != 3 or state.shape[-1] != 4:
        raise RuntimeError(f'lane_follow_step: state must be (B,N,4), got {tuple(state.shape)}')
    B, N = state.shape[:2]
    E = boxes.shape[1]
    check_lane_follow_args(E, dt, horizon, lateral_margin, idm)
    shapes = dict(boxes=(B, E, 5), ent_sc=(B, E, 2), ent_speed=(B, E), ent_present=(B, E), npc_size=(B, N, 2), desired_speed=(B, N), npc_present=(B, N),
                  lane=(B, N), arc=(B, N), hops=(B, N), sc=(B, N, 2), leader=(B, N))
    given = dict(boxes=boxes, ent_sc=ent_sc, ent_speed=ent_speed, ent_present=ent_present, npc_size=npc_size, desired_speed=desired_speed,
                 npc_present=npc_present, lane=lane, arc=arc, hops=hops, sc=sc, leader=leader)
    for k, shp in shapes.items():
        if tuple(given[k].shape) != shp:
            raise RuntimeError(f'lane_follow_step: {k} must be {shp}, got {tuple(given[k].shape)}')
    dev = state.device
    if self_index is not None and tuple(self_index.shape) != (B, N):
        raise RuntimeError(f'lane_follow_step: self_index must be ({B},{N}), got {tuple(self_index.shape)}')
    params = (ctypes.c_float * 5)(*[float(x) for x in idm])
    if stop_at is not None:
        if tuple(stop_at.shape) != (B, N):
            raise RuntimeError(f'lane_follow_step: stop_at must be ({B},{N}), got {tuple(stop_at.shape)}')
        nat.call('tds_lane_follow_step_stops_multi', dev, lane_set.handle, _scene_map(lane_set, B, 'lane_follow_step'), _scene_ids(scene_ids, B, 'lane_follow_step'),
                 B, N, E, _c(boxes), _c(ent_sc), _c(ent_speed), _u8(ent_present), self_index, _c(npc_size), _c(desired_speed), _u8(npc_present), lane, arc, hops,
                 state, sc, leader, stop_at, _seed64(seed), float(dt), float(horizon), float(lateral_margin), params)
        return
    nat.call('tds_lane_follow_step_multi', dev, lane_set.handle, _scene_map(lane_set, B, 'lane_follow_step'), _scene_ids(scene_ids, B, 'lane_follow_step'),
             B, N, E, _c(boxes), _c(ent_sc), _c(ent_speed), _u8(ent_present), self_index, _c(npc_size), _c(desired_speed), _u8(npc_present), lane, arc, hops,
             state, sc, leader, _seed64(seed), float(dt), float(horizon), float(lateral_margin), params)


def check_lane_give_way_args(n_npcs, horizon, b_max, creep_speed):
    """what tds_lane_give_way_multi refuses, refused before any tensor is touched: TdsError with the code the entry point would return"""
    if n_npcs > nat.GIVE_WAY_MAX_NPCS:
        raise nat.TdsError('lane_give_way', nat.E_LIMIT, f'{n_npcs} NPCs exceed the {nat.GIVE_WAY_MAX_NPCS} of a scene\'s workgroup')
    for k, x in (('horizon', horizon), ('b_max', b_max)):
        if not (0.0 <= float(x) < float('inf')):
            raise nat.TdsError('lane_give_way', nat.E_INVAL, f'{k} must be finite and not negative (got {x})')
    if not (0.0 < float(creep_speed) < float('inf')):
        raise nat.TdsError('lane_give_way', nat.E_INVAL, f'creep_speed must be finite and greater than 0 (got {creep_speed})')


def lane_give_way(lane_set, scene_ids, tables, lane, arc, hops, state, npc_size, npc_present, lines, seed, stop_at, yield_to, horizon=60.0, b_max=6.0,
                  creep_speed=1.0):
    """tds_lane_give_way_multi (include/tdship.h): tables = `lane_set.conflict_tables(clearance, step)`; lane / arc / hops (B,N), state (B,N,4),
    npc_size (B,N,2), npc_present (B,N) as `lane_follow_step` takes them; lines = None or (line_lane (B,S) int32, line_arc (B,S) float64, line_red
    (B,S) bool or uint8); stop_at (B,N) float64 and yield_to (B,N) int32 are WRITTEN.  One launch on the current stream, no allocation besides the
    uint8 views of bool masks, no synchronisation."""
    if state.dim() != 3 or state.shape[-1] != 4:
        raise RuntimeError(f'lane_give_way: state must be (B,N,4), got {tuple(state.shape)}')
    B, N = state.shape[:2]
    check_lane_give_way_args(N, horizon, b_max, creep_speed)
    given = dict(lane=lane, arc=arc, hops=hops, npc_size=npc_size, npc_present=npc_present, stop_at=stop_at, yield_to=yield_to)
    for k, t in given.items():
        if tuple(t.shape) != ((B, N, 2) if k == 'npc_size' else (B, N)):
            raise RuntimeError(f'lane_give_way: {k} must be {(B, N, 2) if k == "npc_size" else (B, N)}, got {tuple(t.shape)}')
    if tuple(tables.shape) != (len(lane_set.tables),):
        raise RuntimeError(f'lane_give_way: tables must hold one address per lane table of the set ({len(lane_set.tables)}), got {tuple(tables.shape)}')
    S, line_lane, line_arc, line_red = 0, None, None, None
    if lines is not None:
        line_lane, line_arc, line_red = lines
        S = line_lane.shape[1]
        for k, t in (('line_lane', line_lane), ('line_arc', line_arc), ('line_red', line_red)):
            if tuple(t.shape) != (B, S):
                raise RuntimeError(f'lane_give_way: {k} must be ({B},{S}), got {tuple(t.shape)}')
        line_red = _u8(line_red)
    nat.call('tds_lane_give_way_multi', state.device, lane_set.handle, _scene_map(lane_set, B, 'lane_give_way'), _scene_ids(scene_ids, B, 'lane_give_way'),
             tables, B, N, lane, arc, hops, _c(state), _c(npc_size), _u8(npc_present), S, line_lane, line_arc, line_red, _seed64(seed), float(horizon),
             float(b_max), float(creep_speed), stop_at, yield_to)


# ---------------------------------------------------------------------------------------------------------------
# route goals (csrc/route.hip)
# ---------------------------------------------------------------------------------------------------------------
#: the route tensors of a batch, in the order the entry points take them: name -> (trailing shape, dtype)
ROUTE_TENSORS = (('lanes', (nat.ROUTE_MAX_LANES,), i32), ('n', (), i32), ('start_arc', (), torch.float64), ('end_arc', (), torch.float64),
                 ('offsets', (nat.ROUTE_MAX_LANES,), torch.float64), ('length', (), torch.float64))
ROUTE_STATE = (('cursor', (), i32), ('stored', (), torch.float64), ('completed', (), u8))


def check_route_args(goal_tolerance, off_route_distance, lookahead, spacing):
    """what tds_route_progress_multi refuses, refused before any tensor is touched: TdsError with the code the entry point would return"""
    for k, x in (('goal_tolerance', goal_tolerance), ('off_route_distance', off_route_distance), ('spacing', spacing)):
        if not (0.0 <= float(x) < float('inf')):
            raise nat.TdsError('route_progress', nat.E_INVAL, f'{k} must be finite and not negative (got {x})')
    if not (0 <= int(lookahead) <= nat.ROUTE_MAX_LOOKAHEAD):
        raise nat.TdsError('route_progress', nat.E_INVAL, f'{lookahead} lookahead points, at most {nat.ROUTE_MAX_LOOKAHEAD}')


def _route_tensors(what, route, B, A, names):
    """the named route tensors (dict name -> tensor), each (B, A, ...); that they are dense and of exactly the kernel's type is checked by the call"""
    for name, tail, _ in names:
        if tuple(route[name].shape) != (B, A) + tail:
            raise RuntimeError(f'{what}: route tensor {name} must be {(B, A) + tail}, got {tuple(route[name].shape)}')
    return [route[name] for name, _, _ in names]


def _routes_dealt(route):
    """the kernels write the route tensors behind torch's back: move their version counters on, so that a backward of a step made on the old
    routes (route_progress_grad) can tell.  Host only: no launch."""
    for name, _, _ in ROUTE_TENSORS:
        torch.autograd.graph.increment_version(route[name])


def route_sample(lane_set, scene_ids, lane, arc, distance, present, mask, seed, route):
    """tds_route_sample_multi (include/tdship.h): lane (B,A) int32, arc (B,A) float64, distance (B,A) float64, present / mask (B,A) bool or None;
    `route` (dict of the ROUTE_TENSORS and ROUTE_STATE) is written IN PLACE for the rows of `mask`.  One launch, no allocation besides the
    uint8 views of bool masks, no synchronisation."""
    B, A = lane.shape
    dev = lane.device
    for name, t in (('arc', arc), ('distance', distance)):
        if tuple(t.shape) != (B, A):
            raise RuntimeError(f'route_sample: {name} must be ({B},{A}), got {tuple(t.shape)}')
    masks = []
    for name, t in (('present', present), ('mask', mask)):
        if t is not None and tuple(t.shape) != (B, A):
            raise RuntimeError(f'route_sample: {name} must be ({B},{A}), got {tuple(t.shape)}')
        masks.append(None if t is None else _u8(t))
    nat.call('tds_route_sample_multi', dev, lane_set.handle, _scene_map(lane_set, B, 'route_sample'), _scene_ids(scene_ids, B, 'route_sample'), B, A, lane, arc,
             distance, *masks, _seed64(seed), *_route_tensors('route_sample', route, B, A, ROUTE_TENSORS + ROUTE_STATE))
    _routes_dealt(route)


def route_to(lane_set, lane, arc, dest_lane, dest_arc, present, mask, route):
    """tds_route_to_multi (include/tdship.h): lane, dest_lane (B,A) int32, arc, dest_arc (B,A) float64, present / mask (B,A) bool or None; `route`
    (dict of the ROUTE_TENSORS, ROUTE_STATE and `rest` (B,A) float64) is written IN PLACE for the rows of `mask`.  One launch, no allocation
    besides the uint8 views of bool masks, no synchronisation -- once the set's distance tables exist (`LaneTableSet.distance_tables`)."""
    B, A = lane.shape
    for name, t in (('arc', arc), ('dest_lane', dest_lane), ('dest_arc', dest_arc)):
        if tuple(t.shape) != (B, A):
            raise RuntimeError(f'route_to: {name} must be ({B},{A}), got {tuple(t.shape)}')
    masks = []
    for name, t in (('present', present), ('mask', mask)):
        if t is not None and tuple(t.shape) != (B, A):
            raise RuntimeError(f'route_to: {name} must be ({B},{A}), got {tuple(t.shape)}')
        masks.append(None if t is None else _u8(t))
    nat.call('tds_route_to_multi', lane.device, lane_set.handle, _scene_map(lane_set, B, 'route_to'), lane_set.distance_tables(), B, A, lane, arc, dest_lane,
             dest_arc, *masks, *_route_tensors('route_to', route, B, A, ROUTE_TENSORS + ROUTE_STATE + (('rest', (), torch.float64),)))
    _routes_dealt(route)


def route_progress(lane_set, state, sc, present, route, out, goal_tolerance, off_route_distance, spacing):
    """tds_route_progress_multi: state (B,A,>=2) float32 with dense rows ([x, y] first), sc (B,A,2) [sin, cos], present (B,A) bool or None; the
    route's cursor / stored / completed are updated IN PLACE and `out` (dict: progress, advance, lateral, remaining (B,A) float32, heading
    (B,A,2), reached, off_route (B,A) uint8, lookahead (B,A,K,2)) is written in full.  One launch, no synchronisation."""
    if not state.is_cuda:
        raise RuntimeError(f'route_progress: torchdrivesim_amd kernels run on an MI355X; got a {state.device} tensor (no CPU fallback)')
    if state.dim() != 3 or state.shape[-1] < 2:
        raise RuntimeError(f'route_progress: state must be (B,A,>=2), got {tuple(state.shape)}')
    B, A, S = state.shape
    dev = state.device
    K = out['lookahead'].shape[2]
    check_route_args(goal_tolerance, off_route_distance, K, spacing)
    state = state.detach()
    if state.dtype != f32 or not state.is_contiguous():
        state = _c(state[..., :2])
        S = 2
    sc = _c(sc.detach())
    if tuple(sc.shape) != (B, A, 2):
        raise RuntimeError(f'route_progress: sc must be ({B},{A},2), got {tuple(sc.shape)}')
    if present is not None and tuple(present.shape) != (B, A):
        raise RuntimeError(f'route_progress: present must be ({B},{A}), got {tuple(present.shape)}')
    outs = (('progress', (), f32), ('advance', (), f32), ('lateral', (), f32), ('heading', (2,), f32), ('remaining', (), f32), ('reached', (), u8),
            ('off_route', (), u8), ('lookahead', (K, 2), f32))
    nat.call('tds_route_progress_multi', dev, lane_set.handle, _scene_map(lane_set, B, 'route_progress'), B, A, state, S, sc,
             None if present is None else _u8(present), *_route_tensors('route_progress', route, B, A, ROUTE_TENSORS + ROUTE_STATE), float(goal_tolerance),
             float(off_route_distance), int(K), float(spacing), *_route_tensors('route_progress', out, B, A, outs))


#: the float outputs of a route step, in the order route_progress_grad returns them
ROUTE_FLOATS = ('progress', 'advance', 'lateral', 'heading', 'remaining', 'lookahead')


class _RouteProgressGrad(torch.autograd.Function):
    """the in-place route step as an autograd node: forward = route_progress, backward = tds_route_progress_bwd_multi (csrc/route_bwd.hip)"""

    @staticmethod
    def forward(ctx, state, sc, lane_set, present, route, out, goal_tolerance, off_route_distance, spacing):
        route_progress(lane_set, state, sc, present, route, out, goal_tolerance, off_route_distance, spacing)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(state, sc, route['cursor'].clone())           # the cursor as this launch left it: the next step moves it on
        ctx.lane_set, ctx.present, ctx.spacing = lane_set, present, float(spacing)
        ctx.route = [route[name] for name, _, _ in ROUTE_TENSORS]           # by reference: a route is not copied per step ...
        ctx.versions = [t._version for t in ctx.route]                      # ... so dealing new ones before the backward has to be noticed
        return tuple(out[k].clone() for k in ROUTE_FLOATS)                  # clones: the next step overwrites the buffers

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        state, sc, piece = ctx.saved_tensors
        if [t._version for t in ctx.route] != ctx.versions:
            raise RuntimeError('route_progress_grad: the routes were dealt again (resample / resample_to) between this step and its backward; '
                               'the gradient of a step belongs to the routes it was made on')
        B, A, S = state.shape
        dev = state.device
        xy = state.detach()
        if xy.dtype != f32 or not xy.is_contiguous():                       # as route_progress read it
            xy, S = _c(xy[..., :2]), 2
        K = grads[5].shape[2] if grads[5] is not None else 0
        g_xy, g_sc = torch.empty((B, A, 2), dtype=f32, device=dev), torch.empty((B, A, 2), dtype=f32, device=dev)
        gin = [None if g is None else _c(g) for g in grads]
        nat.call('tds_route_progress_bwd_multi', dev, ctx.lane_set.handle, _scene_map(ctx.lane_set, B, 'route_progress_grad'), B, A, xy, S, _c(sc.detach()),
                 None if ctx.present is None else _u8(ctx.present), *ctx.route, piece, *gin, int(K), ctx.spacing, g_xy, g_sc)
        g_state = None
        if ctx.needs_input_grad[0]:
            extra = state.shape[2] - 2
            g_state = torch.cat([g_xy, _zeros_const((B, A, extra), dev)], dim=-1) if extra else g_xy
            g_state = g_state.to(state.dtype)
        return (g_state, g_sc.to(sc.dtype) if ctx.needs_input_grad[1] else None) + (None,) * 7


def route_progress_grad(lane_set, state, sc, present, route, out, goal_tolerance, off_route_distance, spacing):
    """The route step, differentiable: arguments as `route_progress`, which it launches -- cursor, stored progress and
    `completed` move exactly as there, `out` is written in full -- and CLONES of the six float outputs are returned, in the order of
    ROUTE_FLOATS = (progress, advance, lateral, heading, remaining, lookahead), carrying the graph to `state` ([x, y]; the other columns get
    zeros) and to `sc` = [sin psi, cos psi].  The backward is ONE launch (tds_route_progress_bwd_multi).  The forward's discrete choices are
    constants.  `advance` differentiates as `progress`: the stored progress of the previous step is a constant, so a caller who wants the
    telescoped sum through time differences `progress` itself.  No gradients to the route tensors, no double backward; dealing new routes
    (`route_sample`, `route_to`) between a step and its backward makes that backward raise."""
    if state.dim() != 3 or state.shape[0] * state.shape[1] == 0:
        raise RuntimeError(f'route_progress_grad: state must be a non-empty (B,A,>=2), got {tuple(state.shape)}')
    return _RouteProgressGrad.apply(state, sc, lane_set, present, route, out, goal_tolerance, off_route_distance, spacing)


def route_points(lane_set, route, arcs):
    """tds_route_points_multi: arcs (B,A,Q) -> (B,A,Q,2) float32, the world-frame points at those route arcs"""
    if not arcs.is_cuda:
        raise RuntimeError(f'route_points: torchdrivesim_amd kernels run on an MI355X; got a {arcs.device} tensor (no CPU fallback)')
    B, A = route['n'].shape
    if arcs.dim() != 3 or tuple(arcs.shape[:2]) != (B, A):
        raise RuntimeError(f'route_points: arcs must be ({B},{A},Q), got {tuple(arcs.shape)}')
    Q = arcs.shape[2]
    arcs = _c(arcs.detach(), torch.float64)
    dev = arcs.device
    pts = torch.empty((B, A, Q, 2), dtype=f32, device=dev)
    if B * A * Q == 0:
        return pts
    nat.call('tds_route_points_multi', dev, lane_set.handle, _scene_map(lane_set, B, 'route_points'), B, A, Q,
             *_route_tensors('route_points', route, B, A, ROUTE_TENSORS), arcs, pts)
    return pts
