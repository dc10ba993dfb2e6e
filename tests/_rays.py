"""Seeded ray sets for the ray-query tests (tests/test_rays.py) and tools/rays_bench.py.

BVH-heavy rays: each aims near a BVH primitive from a short distance in a random direction,
so that most of them cross the tree's boxes (a ray from afar mostly hits a wall plane).
"""
import numpy as np

SEED = 20261020
N_FIRST, N_SECOND = 4096, 2048


def bvh_rays(scene, n, rng):
    """n rays: target = the `pos` of a random BVH primitive (dump_bvh's order: planes at the end)
    + N(0, 0.01 x root extent), direction = a random unit vector, origin = target - d x U(0.05, 1)"""
    inf = scene.info
    nodes, prims = scene.dump_bvh()
    root = np.frombuffer(nodes, np.float32, 6)
    extent = float(np.max(root[3:6] - root[0:3]))
    pos = np.frombuffer(prims, np.uint8).reshape(-1, 52)[:inf["n_bvh_prims"], 40:52].copy().view(np.float32)
    target = pos[rng.integers(0, len(pos), n)] + rng.normal(0.0, 0.01 * extent, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = target - d * rng.uniform(0.05, 1.0, (n, 1))
    return np.concatenate([o, d], axis=1).astype(np.float32)


def special_rays(scene, n, rng):
    """n BVH-heavy rays with edits: the first 3/8 get one or two direction components set to +-0
    (the robust box tests), then 8 rays each with d.z = inf, o.x = NaN, d.x = NaN, o.y = -inf,
    d = 0 and d.x = 1e-35 (non-finite rays take the exact DFS; 1e-35 is below the replay's 1e-30)"""
    r = bvh_rays(scene, n, rng)
    k = 3 * n // 8
    for i in range(k):
        for c in rng.choice(3, 1 + i % 2, replace=False):
            r[i, 3 + c] = 0.0 if rng.integers(2) else -0.0
    edits = [(5, np.inf), (0, np.nan), (3, np.nan), (1, -np.inf), (None, 0.0), (3, 1e-35)]
    for j, (col, val) in enumerate(edits):
        rows = slice(k + 8 * j, k + 8 * j + 8)
        if col is None:
            r[rows, 3:6] = val
        else:
            r[rows, col] = val
    return r


def ray_sets(scene):
    """(first set, second set) of a scene, from one generator seeded with SEED"""
    rng = np.random.default_rng(SEED)
    return bvh_rays(scene, N_FIRST, rng), special_rays(scene, N_SECOND, rng)


def expected_hits(pt, ids, f, interior):
    """reference answers (id, {t, n.xyz}, interior) as an array of HIT_DTYPE; misses all zero but id"""
    h = np.zeros(len(ids), pt.HIT_DTYPE)
    hit = ids != -1
    h["id"] = np.where(hit, ids, -1)
    h["t"][hit] = f[hit, 0]
    h["n"][hit] = f[hit, 1:4]
    h["interior"][hit] = np.asarray(interior)[hit].astype(np.uint32)
    return h
