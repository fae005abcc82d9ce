"""What the CPU and the GPU tests of giving way share: a synthetic four-way crossing, scenes stepped on the model alone, rectangle overlaps."""
import math

import numpy as np

import give_way_model as gw
import lane_follow_model as lf

F32 = np.float32
ARM, HALF_BOX, LANE = 60.0, 7.0, 3.5            # metres: an approach, half the junction's square, a lane's width
STREAMS = ('east', 'north', 'west', 'south')   # the direction of travel; stream d is stream 0 turned by d quarter turns
SIZE = (4.5, 2.0)


def crossing_map():
    """Four one-lane streams straight across a square junction (right-hand traffic, no turns): per stream an approach of ARM metres, a
    junction lanelet of 2 HALF_BOX and an exit of ARM, joined through shared bound point ids -> lanelets 3 d + (0, 1, 2) of stream d.  Every
    coordinate is a binary fraction and stream d is stream 0 turned by d quarter turns, so the four streams' numbers are bit-equal.
    By hand: the centre lines run 1.75 m beside the axes; a junction lanelet crosses the stream from its left 5.25 m and the stream from its
    right 8.75 m after its start, and its samples (every 0.5 m) within 2.0 m of them are 3.5 .. 7.0 and 7.0 .. 10.5; opposite streams are
    3.5 m apart and never within 2.0 m.  So 4 lanelets conflict, in 8 ordered pairs, 2 each; zone_in = 3.5 and zone_out = 10.5."""
    from torchdrivesim_amd import lanelet2
    out = []
    xs = [-HALF_BOX - ARM, -HALF_BOX, HALF_BOX, HALF_BOX + ARM]
    for d in range(4):
        turn = lambda p: [(p[0], p[1]), (-p[1], p[0]), (-p[0], -p[1]), (p[1], -p[0])][d]
        for i in range(3):
            left = np.array([turn((xs[i], 0.0)) + (0.0,), turn((xs[i + 1], 0.0)) + (0.0,)])
            right = np.array([turn((xs[i], -LANE)) + (0.0,), turn((xs[i + 1], -LANE)) + (0.0,)])
            base = 100 * d + 2 * i
            out.append(lanelet2.Lanelet(3 * d + i + 1, left, right, np.array([base, base + 2]), np.array([base + 1, base + 3]), {'type': 'lanelet'}))
    return lanelet2.LaneletMap([], np.zeros((0, 3)), out)


def rectangles_overlap(a, b):
    """two boxes [x, y, length, width, psi]: the separating-axis test, touching counts as apart"""
    def corners(r):
        c, s = math.cos(r[4]), math.sin(r[4])
        return [(r[0] + fl * c - fw * s, r[1] + fl * s + fw * c) for fl, fw in ((r[2] / 2, r[3] / 2), (r[2] / 2, -r[3] / 2), (-r[2] / 2, -r[3] / 2), (-r[2] / 2, r[3] / 2))]
    ca, cb = corners(a), corners(b)
    for r in (a, b):
        for ax in ((math.cos(r[4]), math.sin(r[4])), (-math.sin(r[4]), math.cos(r[4]))):
            pa, pb = [x * ax[0] + y * ax[1] for x, y in ca], [x * ax[0] + y * ax[1] for x, y in cb]
            if max(pa) <= min(pb) + 1e-9 or max(pb) <= min(pa) + 1e-9:
                return False
    return True


class Scene:
    """N NPCs on one map stepped by the model alone (no other entities): what a controller with N NPCs and no exposed agents does"""

    def __init__(self, lanes, placements, seed=1, scene_id=0, v0=8.0, size=SIZE, dt=0.1, give_way=True, tables=None, lines=()):
        self.lanes, self.seed, self.scene_id, self.dt, self.give_way, self.lines = lanes, seed, scene_id, dt, give_way, list(lines)
        self.tables = tables if tables is not None else gw.conflict_tables(lanes)
        N = len(placements)
        self.lane = np.array([p[0] for p in placements], np.int32)
        self.arc = np.array([p[1] for p in placements], np.float64)
        self.hops = np.zeros(N, np.int32)
        self.size = np.tile(np.array(size, F32), (N, 1))
        self.v0 = np.full(N, v0, F32)
        self.present = np.ones(N, bool)
        self.state, self.sc = np.zeros((N, 4), F32), np.zeros((N, 2), F32)
        for n, p in enumerate(placements):
            x, y, psi, sn, cs = lanes.pose(int(p[0]), float(p[1]))
            self.state[n], self.sc[n] = (x, y, psi, p[2]), (sn, cs)
        self.leader, self.stop_at, self.yield_to = np.full(N, -1), np.full(N, np.inf), np.full(N, -1)

    def boxes(self):
        return np.concatenate([self.state[:, :2], self.size, self.state[:, 2:3]], 1).astype(F32)

    def step(self):
        N = len(self.lane)
        args = (self.lane, self.arc, self.hops, self.state, self.size, self.v0, self.present, self.boxes(), self.sc, self.state[:, 3].copy(), self.present,
                np.arange(N), self.seed, self.scene_id, self.dt)
        if self.give_way:
            out = gw.step_scene(self.lanes, self.tables, *args, lines=self.lines)
            self.stop_at, self.yield_to = out['stop_at'], out['yield_to']
        else:
            out = lf.step_scene(self.lanes, *args)
        self.lane, self.arc, self.hops, self.state, self.leader = out['lane'], out['arc'], out['hops'], out['state'], out['leader']
        self.sc = np.where(out['moved'][:, None], out['sc'], self.sc)
        return out

    def overlaps(self):
        b = self.boxes().astype(np.float64)
        return [(i, j) for i in range(len(b)) for j in range(i + 1, len(b)) if self.present[i] and self.present[j] and rectangles_overlap(b[i], b[j])]
