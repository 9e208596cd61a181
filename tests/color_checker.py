"""Sequential restatement of the colour half of lioOptimization::addPointsToMap (src/lioOptimization.cpp:520-554): addPointToColorMap
(:448-518) for every add_point_step-th frame point, into color_voxel_map, rgb_points_vec, hashmap_3d_points (include/utility.h:94-141)
and voxels_recent_visited_temp.  One point after the other, plain dictionaries, no cleverness: what the device map (srl_color_map_*)
and the recorded golden file are compared with, and what tests/test_color_checker_reference.py pins to the reference's own
translation units bit for bit.  The times are explicit arguments.

Also the scene of the tests (scene_batch): ground, a wall, a small dense box that fills voxels and collides in the 1 cm grid, the same box
655.36 m away in x (the 16-bit wrap of the grid key makes the two share cells) and a handful of points near the origin.
"""
import numpy as np

OPTION_SETS = ((0.1, 50, 0.01, 1), (0.1, 20, 0.01, 4), (0.25, 50, 0.05, 1), (0.1, 5, 0.02, 1))      # size, cap, grid, step
STORED_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("kx", "<i2"), ("ky", "<i2"), ("kz", "<i2"), ("slot", "<u2"),
                         ("batch_index", "<i4"), ("point_index", "<i4")])


def short_keys(p32, size):
    """static_cast<short>(float / double) per axis (:453-459): FP64 division of the FP32 value, truncation, 16-bit wrap"""
    q = np.trunc(p32.astype(np.float64) / np.float64(size)).astype(np.int64)
    return ((q + 32768) % 65536 - 32768).astype(np.int16)


def scene_batch(j):
    rng = np.random.default_rng(9100 + j)
    c = 0.3 * j
    ground = np.stack([rng.uniform(-12, 12, 6000) + c, rng.uniform(-12, 12, 6000), -1.7 + 0.02 * rng.standard_normal(6000)], 1)
    wall = np.stack([6 + c + 0.02 * rng.standard_normal(1500), rng.uniform(-12, 12, 1500), rng.uniform(-1.7, 2.0, 1500)], 1)
    box = np.stack([rng.uniform(5, 5.3, 2500), rng.uniform(5, 5.3, 2500), rng.uniform(0, 0.1, 2500)], 1)
    alias = np.stack([rng.uniform(5, 5.3, 900) - 655.36, rng.uniform(5, 5.3, 900), rng.uniform(0, 0.1, 900)], 1)
    near = 0.2 * rng.standard_normal((300, 3))
    pts = np.concatenate([ground, wall, box, alias, near])
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


class Voxel:
    __slots__ = ("key", "points", "point_index", "last_visited_time")

    def __init__(self, key):
        self.key = key
        self.points = []                 # FP32 triples in slot order
        self.point_index = []            # index in rgb_points_vec or -1
        self.last_visited_time = 0.0     # cloudMap.h:153


class ColorChecker:
    def __init__(self, size_voxel_map=0.1, max_num_points_in_voxel=50, min_distance_points=0.01, add_point_step=1):
        self.size, self.cap, self.grid_size, self.step = float(size_voxel_map), int(max_num_points_in_voxel), float(min_distance_points), int(add_point_step)
        self.voxels = {}                 # key -> Voxel; dict order = creation order
        self.grid = {}                   # grid key -> index in the registered list (hashmap_3d_points)
        self.registered = []             # rgb_points_vec: (x, y, z, voxel key, slot)
        self.num_points = 0
        # branch counters over the map's life (the tests assert each > 0 on their scene)
        self.n_refused_full = 0
        self.n_stored_not_registered = 0
        self.n_stored_not_registered_other_voxel = 0     # ... whose grid cell belongs to a point of ANOTHER voxel (the 16-bit wrap)
        self.n_registered_after_unstored = 0             # registered although an earlier point of the same cell was refused
        self.n_created = 0
        self.n_retouched = 0                             # voxels touched in a batch that existed before it
        self._unstored_cells = set()

    def insert(self, world_xyz, time_sweep_end, time_last_process=0.0):
        """Returns outcome (n uint8: bit 0 stored, bit 1 created, bit 2 registered), the stored records (STORED_DTYPE, batch order) and the
        batch's visited list (m x 3 int32, order of first touch)."""
        w = np.ascontiguousarray(world_xyz, dtype=np.float64).reshape(-1, 3)
        n = len(w)
        p32 = w.astype(np.float32)                       # rgbPoint(point.point): cloudMap.cpp:7
        k = short_keys(p32, self.size)
        g = short_keys(p32, self.grid_size)
        outcome = np.zeros(n, np.uint8)
        stored, visited = [], []
        existed_before = set(self.voxels)
        touched_old = set()
        for i in range(0, n, self.step):                 # :538
            key = (int(k[i, 0]), int(k[i, 1]), int(k[i, 2]))
            cell = (int(g[i, 0]), int(g[i, 1]), int(g[i, 2]))
            add_point = cell not in self.grid            # :461-462
            vox = self.voxels.get(key)
            bits = 0
            if vox is None:                              # :493-516
                vox = self.voxels[key] = Voxel(key)
                bits |= 2
                self.n_created += 1
                do_store = True
            else:                                        # :466-491
                do_store = len(vox.points) < self.cap    # IsFull(); min_num_points is 0 (:539)
                if key in existed_before:
                    touched_old.add(key)
            if do_store:
                slot = len(vox.points)
                vox.points.append((p32[i, 0], p32[i, 1], p32[i, 2]))
                idx = -1
                if add_point:                            # :476-483, :501-508
                    idx = len(self.registered)
                    self.registered.append((p32[i, 0], p32[i, 1], p32[i, 2], key, slot))
                    self.grid[cell] = idx
                    bits |= 4
                    if cell in self._unstored_cells:
                        self.n_registered_after_unstored += 1
                else:
                    self.n_stored_not_registered += 1
                    if self.registered[self.grid[cell]][3] != key:
                        self.n_stored_not_registered_other_voxel += 1
                vox.point_index.append(idx)
                self.num_points += 1
                bits |= 1
                stored.append((p32[i, 0], p32[i, 1], p32[i, 2], key[0], key[1], key[2], slot, i, idx))
            else:
                self.n_refused_full += 1
                if add_point:
                    self._unstored_cells.add(cell)
            if abs(time_sweep_end - time_last_process) > 1e-5 and abs(vox.last_visited_time - time_sweep_end) > 1e-5:      # :487-491, :510-514
                vox.last_visited_time = time_sweep_end
                visited.append(key)
            outcome[i] = bits
        self.n_retouched += len(touched_old)
        rec = np.array(stored, dtype=STORED_DTYPE) if stored else np.zeros(0, STORED_DTYPE)
        return outcome, rec, np.array(visited, dtype=np.int32).reshape(-1, 3)

    # what the downloads of the device map give
    def sizes(self):
        return self.num_points, len(self.voxels), len(self.registered), len(self.grid)

    def map_arrays(self):
        keys = np.array([v.key for v in self.voxels.values()], dtype=np.int16).reshape(-1, 3)
        counts = np.array([len(v.points) for v in self.voxels.values()], dtype=np.int32)
        times = np.array([v.last_visited_time for v in self.voxels.values()], dtype=np.float64)
        xyz = np.array([p for v in self.voxels.values() for p in v.points], dtype=np.float32).reshape(-1, 3)
        pidx = np.array([q for v in self.voxels.values() for q in v.point_index], dtype=np.int32)
        return keys, counts, times, xyz, pidx

    def registered_arrays(self):
        xyz = np.array([r[:3] for r in self.registered], dtype=np.float32).reshape(-1, 3)
        keys = np.array([r[3] for r in self.registered], dtype=np.int16).reshape(-1, 3)
        slot = np.array([r[4] for r in self.registered], dtype=np.int32)
        return xyz, keys, slot
