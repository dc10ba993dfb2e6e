"""Scenes for the vertex step's light sampling (test_light_sampling.py on the GPU,
test_light_sampling_host.py on the host): 16 x 16 pixels, 4 samples, RAY_DEPTH 6, every
surface diffuse so that every hit samples a direction (sample_mix_e) and takes its pdf
(pdf_mix_e).

The surfaces are one of each kind a closest hit can name: a plane without and with a
rotation, a triangle as written, one moved by POSITION, one rotated, a box without and with a
rotation, a rotated ellipsoid.  The emitters:
  none   no emitter: every vertex samples the cosine distribution (three normals, from one or
         two polar pairs according to the saved value the pixel's stream carries); light comes
         from the background.
  box    one axis-aligned box: a light lane's accepting hit and a cosine lane's first pdf point
         are both emitter 0's.
  two    a rotated box and an ellipsoid: the hit that the sampler hands to the pdf belongs to
         emitter 0 for the cosine lanes and for some light lanes, to emitter 1 for the others,
         and the pdf tests the other emitter itself.  The ellipsoid's candidates draw normals.
"""
W, H, SPP, DEPTH = 16, 16, 4, 6

HEAD = """DIMENSIONS %d %d
RAY_DEPTH %d
SAMPLES %d

BG_COLOR %%s

CAMERA_POSITION 0 0 0
CAMERA_RIGHT 1 0 0
CAMERA_UP 0 1 0
CAMERA_FORWARD 0 0 -1
CAMERA_FOV_X 1.2
""" % (W, H, DEPTH, SPP)

SURFACES = """
NEW_PRIMITIVE
PLANE 0 1 0
POSITION 0 -2 0
COLOR 0.8 0.8 0.8

NEW_PRIMITIVE
PLANE 0 0 1
POSITION 0 0 -5
ROTATION 0 0.1305262 0 0.9914449
COLOR 0.7 0.8 0.9

NEW_PRIMITIVE
TRIANGLE -2 -1 -4 -0.5 -1 -4 -1.2 0.5 -4.2
COLOR 0.9 0.5 0.4

NEW_PRIMITIVE
TRIANGLE 0 0 0 1 0 0 0 1 0
POSITION 0.5 -0.5 -3
COLOR 0.4 0.9 0.5

NEW_PRIMITIVE
TRIANGLE 0 0 0 1 0 0 0 1 0
POSITION -0.5 0.5 -2.5
ROTATION 0 0.3826834 0 0.9238795
COLOR 0.8 0.6 0.4

NEW_PRIMITIVE
BOX 0.3 0.2 0.4
POSITION 0.8 -1.2 -2.5
COLOR 0.5 0.5 1.0

NEW_PRIMITIVE
BOX 0.3 0.3 0.3
POSITION -1 -1.3 -3
ROTATION 0 0.2588190 0 0.9659258
COLOR 1.0 0.9 0.5

NEW_PRIMITIVE
ELLIPSOID 0.5 0.3 0.4
POSITION 0 0.8 -3.5
ROTATION 0.2588190 0 0 0.9659258
COLOR 0.9 0.9 0.9
"""

# emitter variant -> (background, emitters): without an emitter the background is the light
EMITTERS = {
    "none": ("0.1 0.2 0.3", ""),
    "box": ("0 0 0", """
NEW_PRIMITIVE
BOX 0.4 0.05 0.4
POSITION 0 2 -3
COLOR 0 0 0
EMISSION 30 30 30
"""),
    "two": ("0 0 0", """
NEW_PRIMITIVE
BOX 0.4 0.05 0.3
POSITION -0.5 2 -3
ROTATION 0 0 0.2588190 0.9659258
COLOR 0 0 0
EMISSION 30 30 30

NEW_PRIMITIVE
ELLIPSOID 0.2 0.15 0.2
POSITION 1.5 1 -2.5
COLOR 0 0 0
EMISSION 20 25 30
"""),
}


def scene_text(variant):
    bg, em = EMITTERS[variant]
    return HEAD % bg + SURFACES + em


def write_scene(tmp_path, variant):
    path = str(tmp_path / ("mixed_%s.txt" % variant))
    with open(path, "w") as f:
        f.write(scene_text(variant))
    return path


def assert_light_reached(orad, octr):
    """From the oracle's image: paths went on past their first vertex (a direction was
    sampled and accepted), and light came back along them to most pixels."""
    assert octr["rays"] > W * H * SPP
    lit = (orad.reshape(-1, 3) > 0).any(axis=1)
    assert lit.sum() >= W * H // 2
