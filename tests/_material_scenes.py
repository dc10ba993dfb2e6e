"""Scenes and rays for the material / primitive-edge tests (test_materials_host.py on the
host, test_materials.py on the GPU; recorded from the reference by tests/golden/make_golden.py
as the fixtures `material:<name>` names).  Everything here is deterministic text and numbers.

Render scenes (at most 24 x 24 pixels, 8 samples, RAY_DEPTH 8):
  matrix  a room of planes -- the back wall METALLIC with a ROTATION, the left wall a
          DIELECTRIC of IOR 0.7 and the floor one of IOR 1.5, each with a diffuse plane behind
          it -- and a box emitter under the ceiling.  Inside: a glass and a metal box and ellipsoid, each with a ROTATION;
          glass and metal triangles with POSITION and with POSITION + ROTATION (the glass
          one with both has IOR 0.7); a glass triangle as written, in a plane through the
          origin, so that the copy the renderer hits is the triangle itself; an ellipsoid of
          IOR 1.0; a METALLIC ellipsoid that is also an emitter.
  inside  the camera inside a rotated glass box inside a large glass ellipsoid, a metal
          ellipsoid in the box with it: first hits are interior ones, and total internal
          reflection is common.
  camera  the matrix content at 23 x 17 pixels through a camera whose axes are neither
          axis-aligned nor of unit length.
Ray scene:
  edges   power-of-two sizes and positions, and rotations that only permute or negate the
          axes, so that the ties the rays aim at really occur in float arithmetic.

Every primitive carries a POSITION line, the triangle "as written" a POSITION 0 0 0: without
one the reference leaves the position indeterminate, which no fixture can pin.
"""
import numpy as np

PREFIX = "material:"
RENDER = ("matrix", "inside", "camera")
N_RAYS = 4096
SEED = 20261020

_HEAD = """DIMENSIONS %d %d
RAY_DEPTH 8
SAMPLES 8

BG_COLOR %s

CAMERA_POSITION %s
CAMERA_RIGHT %s
CAMERA_UP %s
CAMERA_FORWARD %s
CAMERA_FOV_X %s
"""

_MATRIX_HEAD = _HEAD % (24, 24, "0 0 0", "0 0 4.5", "1 0 0", "0 1 0", "0 0 -1", "1.1")
_CAMERA_HEAD = _HEAD % (23, 17, "0 0 0", "-0.4 0.3 4.5", "0.9 0.1 -0.3", "-0.05 1.1 0.1", "0.15 -0.05 -0.8", "1.3")

_MATRIX_BODY = """
NEW_PRIMITIVE
PLANE 0 1 0
POSITION 0 -2.5 0
COLOR 0.8 0.8 0.8

NEW_PRIMITIVE
PLANE 0 1 0
POSITION 0 -2 0
DIELECTRIC
IOR 1.5
COLOR 0.95 0.95 0.9

NEW_PRIMITIVE
PLANE 0 -1 0
POSITION 0 2 0
COLOR 0.8 0.8 0.8

NEW_PRIMITIVE
PLANE 0 0 1
POSITION 0 0 -2.5
ROTATION 0 0.0871557 0 0.9961947
METALLIC
COLOR 0.9 0.8 0.6

NEW_PRIMITIVE
PLANE 1 0 0
POSITION -2 0 0
DIELECTRIC
IOR 0.7
COLOR 0.8 0.9 1.0

NEW_PRIMITIVE
PLANE 1 0 0
POSITION -3 0 0
COLOR 0.9 0.6 0.5

NEW_PRIMITIVE
PLANE -1 0 0
POSITION 2 0 0
COLOR 0.5 0.8 0.5

NEW_PRIMITIVE
PLANE 0 0 -1
POSITION 0 0 5
COLOR 0.8 0.8 0.8

NEW_PRIMITIVE
BOX 0.6 0.05 0.6
POSITION 0 1.95 0.5
COLOR 0 0 0
EMISSION 25 25 25

NEW_PRIMITIVE
BOX 0.45 0.45 0.45
POSITION -1.1 -1.3 0.6
ROTATION 0 0.2588190 0 0.9659258
DIELECTRIC
IOR 1.5
COLOR 0.9 0.95 1.0

NEW_PRIMITIVE
BOX 0.35 0.5 0.3
POSITION 1.3 -1.4 -0.6
ROTATION 0.1305262 0.2588190 0 0.9569403
METALLIC
COLOR 0.9 0.7 0.5

NEW_PRIMITIVE
ELLIPSOID 0.7 0.4 0.45
POSITION 0.9 -0.2 1.0
ROTATION 0 0 0.3826834 0.9238795
DIELECTRIC
IOR 2.4
COLOR 1.0 0.9 0.9

NEW_PRIMITIVE
ELLIPSOID 0.5 0.35 0.4
POSITION -0.9 0.9 -0.8
ROTATION 0.2588190 0 0 0.9659258
METALLIC
COLOR 0.7 0.8 0.9

NEW_PRIMITIVE
ELLIPSOID 0.4 0.4 0.3
POSITION 0.2 -1.5 1.6
DIELECTRIC
IOR 1.0
COLOR 0.9 1.0 0.9

NEW_PRIMITIVE
ELLIPSOID 0.25 0.2 0.25
POSITION 1.4 1.2 0.4
METALLIC
COLOR 0.9 0.9 0.9
EMISSION 6 5 4

NEW_PRIMITIVE
TRIANGLE -0.7 -0.6 0 0.7 -0.6 0 0 0.7 0
POSITION -0.9 -0.2 1.8
DIELECTRIC
IOR 2.4
COLOR 0.9 0.9 1.0

NEW_PRIMITIVE
TRIANGLE -0.9 -0.7 0 0.9 -0.7 0 0 0.9 0
POSITION 0.1 0.9 1.2
ROTATION 0.5 0 0 0.8660254
DIELECTRIC
IOR 0.7
COLOR 1.0 0.9 0.8

NEW_PRIMITIVE
TRIANGLE -0.6 -0.5 0 0.6 -0.5 0 0 0.6 0
POSITION 1.2 0.5 -1.2
METALLIC
COLOR 0.8 0.8 0.9

NEW_PRIMITIVE
TRIANGLE -0.6 -0.5 0 0.6 -0.5 0 0 0.6 0
POSITION -0.3 -0.9 -0.9
ROTATION 0 0.3826834 0 0.9238795
METALLIC
COLOR 0.9 0.8 0.8

NEW_PRIMITIVE
TRIANGLE -0.6 -1.9 0 0.6 -1.9 0 0 -0.6 0
POSITION 0 0 0
DIELECTRIC
IOR 1.5
COLOR 0.9 1.0 1.0
"""

_INSIDE = _HEAD % (24, 24, "0.5 0.6 0.8", "0 0 0.4", "1 0 0", "0 1 0", "0 0 -1", "1.4") + """
NEW_PRIMITIVE
BOX 0.9 0.7 0.8
POSITION 0 0 0
ROTATION 0.1305262 0.2588190 0 0.9569403
DIELECTRIC
IOR 1.5
COLOR 0.9 0.95 1.0

NEW_PRIMITIVE
ELLIPSOID 2.5 2.0 3.0
POSITION 0.2 0.1 -0.3
DIELECTRIC
IOR 1.3
COLOR 1.0 0.9 0.8

NEW_PRIMITIVE
ELLIPSOID 0.25 0.2 0.15
POSITION 0.1 -0.1 -0.3
ROTATION 0 0 0.2588190 0.9659258
METALLIC
COLOR 0.9 0.7 0.4

NEW_PRIMITIVE
BOX 0.5 0.5 0.1
POSITION 0 0 -5
COLOR 0 0 0
EMISSION 12 12 12

NEW_PRIMITIVE
PLANE 0 1 0
POSITION 0 -4 0
COLOR 0.7 0.7 0.7
"""

# ---- the edge scene ---------------------------------------------------------------------------
# (kind, size rows, position, rotation x y z w): the rotations permute or negate axes exactly
_EDGE_PRIMS = [
    ("BOX", [(0.5, 0.25, 0.5)], (-2.0, 0.0, 0.0), None),
    ("BOX", [(0.5, 0.25, 1.0)], (2.0, 0.0, 0.0), (0.5, 0.5, 0.5, 0.5)),
    ("ELLIPSOID", [(0.5, 0.5, 0.5)], (0.0, 2.0, 0.0), None),
    ("ELLIPSOID", [(1.0, 0.5, 0.25)], (0.0, -2.0, 0.0), None),
    ("TRIANGLE", [(-0.5, -0.5, 0.25), (0.5, -0.5, 0.25), (0.0, 0.5, 0.25)], (0.0, 0.0, 0.0), None),
    ("TRIANGLE", [(0.0, 0.0, 0.125), (1.0, 0.0, 0.125), (0.0, 1.0, 0.125)], (2.0, 2.0, 0.0), None),
    ("PLANE", [(0.0, 1.0, 0.0)], (0.0, -4.0, 0.0), None),
    ("PLANE", [(0.0, 0.0, 1.0)], (0.0, 0.0, -4.0), (0.0, 1.0, 0.0, 0.0)),
]


def _edges_text():
    out = [_HEAD % (8, 8, "0 0 0", "0 0 8", "1 0 0", "0 1 0", "0 0 -1", "1.0")]
    for kind, rows, pos, rot in _EDGE_PRIMS:
        out.append("NEW_PRIMITIVE")
        out.append(kind + " " + " ".join("%g" % v for r in rows for v in r))
        if pos is not None:
            out.append("POSITION %g %g %g" % pos)
        if rot is not None:
            out.append("ROTATION %g %g %g %g" % rot)
        out.append("COLOR 0.5 0.5 0.5\n")
    return "\n".join(out)


def scene_text(name):
    if name == "matrix":
        return _MATRIX_HEAD + _MATRIX_BODY
    if name == "camera":
        return _CAMERA_HEAD + _MATRIX_BODY
    if name == "inside":
        return _INSIDE
    if name == "edges":
        return _edges_text()
    raise KeyError(name)


# ---- the edge rays ------------------------------------------------------------------------------
def _qrot(q, v):
    x, y, z, w = q
    u = np.array([x, y, z])
    uv = np.cross(u, v)
    return v + 2.0 * (w * uv + np.cross(u, uv))


def _world(p, pos, rot):
    p = np.asarray(p, np.float64)
    if rot is not None:
        p = _qrot(rot, p)
    if pos is not None:
        p = p + np.asarray(pos, np.float64)
    return p


def edge_targets():
    """Points on the edge scene's primitives at which a primitive test decides by a tie or a
    sign: box corners, edge midpoints and face centres; the ellipsoids' axis points (every
    direction at right angles to the axis is a tangent there); the vertices and edge midpoints
    of each triangle and of its copy on the plane through its local origin, and the points a
    quarter of the way from those to the centroid.  Returns (points, index into _EDGE_PRIMS)."""
    pts, owner = [], []
    for ip, (kind, rows, pos, rot) in enumerate(_EDGE_PRIMS):
        n0 = len(pts)
        if kind == "BOX":
            s = np.array(rows[0])
            for i in (-1, 0, 1):
                for j in (-1, 0, 1):
                    for k in (-1, 0, 1):
                        if (i, j, k) != (0, 0, 0):
                            pts.append(_world(s * (i, j, k), pos, rot))
        elif kind == "ELLIPSOID":
            r = np.array(rows[0])
            for a in range(3):
                for sgn in (-1.0, 1.0):
                    e = np.zeros(3)
                    e[a] = sgn * r[a]
                    pts.append(_world(e, pos, rot))
        elif kind == "TRIANGLE":
            a, b, c = (np.array(v) for v in rows)
            n = np.cross(b - a, c - a)
            n /= np.linalg.norm(n)
            g = (a + b + c) / 3
            rim = (a, b, c, (a + b) / 2, (b + c) / 2, (c + a) / 2)
            for v in rim + tuple(0.75 * v + 0.25 * g for v in rim) + (g,):
                pts.append(_world(v, pos, rot))
                pts.append(_world(v - n * np.dot(v, n), pos, rot))   # its copy on the plane through the origin
        owner += [ip] * (len(pts) - n0)
    return np.array(pts), np.array(owner)


def _directions():
    d = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)]
    d += [(1, 2, -3), (-0.5, 0.25, 1), (3, -1, 0.125), (0.1, -0.7, 0.3)]
    return np.array(d, np.float64)


def _plane_rays():
    """Rays in and parallel to each plane (0 / 0 and x / 0 in the plane test), and rays that hit
    the plane y = -4 at t on both sides of 1e5: the float 1e5, its two neighbours, and further."""
    rays = []
    par = [(1, 0, 0), (0, 0, 1), (1, 0, -1), (-1, 0, 0.5), (0, 0, -1)]
    for y in (-4.0, -3.0, -5.0, np.nextafter(np.float32(-4), np.float32(0)), np.nextafter(np.float32(-4), np.float32(-8))):
        for d in par:
            for o in ((0, y, 0), (-2, y, 0), (0.3, y, -1.7)):
                rays.append(o + d)
                rays.append(o + (d[0], -0.0, d[2]))
    for z in (-4.0, -3.0, -5.0):
        for d in ((1, 0, 0), (0, 1, 0), (1, -1, 0), (-1, 0.5, 0)):
            for o in ((0, 0, z), (0, -2, z), (1.7, 0.3, z)):
                rays.append(o + d)
    # o one above the plane, d = (0, -k, 0): t = 1 / k in float arithmetic
    t5 = np.float32(1e5)
    want = [t5, np.nextafter(t5, np.float32(0)), np.nextafter(t5, np.float32(2e5)), np.float32(99999), np.float32(100001),
            np.float32(5e4), np.float32(2e5), np.float32(1e6)]
    for t in want:
        k0 = np.float32(1) / t
        k = k0
        for step in range(-8, 9):   # the k whose quotient is exactly t, where there is one
            c = np.float32(k0)
            for _ in range(abs(step)):
                c = np.nextafter(c, np.float32(1 if step > 0 else 0))
            if np.float32(1) / c == t:
                k = c
                break
        for o in ((0, -3, 0), (-2, -3, 0), (0.3, -3, -1.7), (0, -5, 0)):
            s = 1.0 if o[1] > -4 else -1.0
            rays.append(o + (0.0, -s * float(k), 0.0))
            rays.append(o + (float(k), -s * float(k), 0.0))
    return np.array(rays, np.float64)


def edge_rays():
    """Exactly N_RAYS rays (float32, n x 6: origin, direction as given, not normalised): all the
    plane rays, and a seeded selection, a fixed share for every primitive (a triangle's twice a
    solid's: most rays at its rim miss), of the rays through its edge targets -- aimed at them from 2 before, started on them, at 1e-4 before and at
    0.25 past -- of which every fifth has one origin component moved by one ulp; in a seeded
    order."""
    rng = np.random.default_rng(SEED)
    (T, owner), D = edge_targets(), _directions()
    starts = (-2.0, 0.0, -1e-4, 0.25)
    o = (T[:, None, None, :] + D[None, :, None, :] * np.array(starts)[None, None, :, None])
    d = np.broadcast_to(D[None, :, None, :], o.shape)
    aimed = np.concatenate([o.reshape(-1, 3), d.reshape(-1, 3)], axis=1).astype(np.float32)
    plane = _plane_rays().astype(np.float32)
    owner = np.repeat(owner, len(D) * len(starts))
    prims = np.unique(owner)
    share = np.array([2 if _EDGE_PRIMS[p][0] == "TRIANGLE" else 1 for p in prims])
    quota = (N_RAYS - len(plane)) * share // share.sum()
    quota[:(N_RAYS - len(plane)) - quota.sum()] += 1
    keep = np.sort(np.concatenate([rng.permutation(np.nonzero(owner == p)[0])[:q] for p, q in zip(prims, quota)]))
    aimed = aimed[keep]
    for i in range(0, len(aimed), 5):
        c = int(rng.integers(3))
        aimed[i, c] = np.nextafter(aimed[i, c], np.float32(rng.choice([-1e9, 1e9])))
    rays = np.concatenate([plane, aimed])
    rays = np.ascontiguousarray(rays[rng.permutation(N_RAYS)])   # any leading part holds every sort
    assert rays.shape == (N_RAYS, 6) and rays.dtype == np.float32
    return rays
