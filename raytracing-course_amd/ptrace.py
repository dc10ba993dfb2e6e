"""ptrace -- Python host mirror of the hw5 render path over libpt.so (ctypes).

Mirrors the reference's in-process interface (hw5/include/scene.h:76-79):

    Scene.load(path)      <- Scene::Load(std::istream&)   (src/sceneload.cpp:112-176)
    scene.prepare()       <- Scene::InitScene()            (src/scene.cpp:7-40)
    scene.render(...)     <- Scene::Render(std::ostream&)  (src/scene.cpp:205-252)
    write_ppm(path, img)  <- the P6 write inside Render    (src/scene.cpp:206-208,243-251)

plus `Session` (tile-sharded progressive rendering on one GPU, used by bench.py
with one process per GPU).  Everything runs through the C ABI of
include/pt.h; there is no Python or CPU fallback: if libpt.so is missing the
import fails, and rendering without a gfx950 GPU raises PTError(PT_E_NO_GPU).
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PT_LIB", os.path.join(HERE, "build", "libpt.so"))

PT_OK = 0
PT_E_INVALID, PT_E_IO, PT_E_SCENE, PT_E_NO_GPU, PT_E_HIP, PT_E_RCCL, PT_E_OOM = -1, -2, -3, -4, -5, -6, -7
TRAVERSAL_REPLAY = 0
TRAVERSAL_EXACT = 1
TRAVERSAL_REPLAY_DIV = 2
GATHER_AUTO, GATHER_RCCL, GATHER_HOST = 0, 1, 2
# pt_stats.handoff sites, in PT_HO_* order (include/pt.h; PT_TUNE drop=<name>)
HANDOFF_SITES = ("suspend", "flush", "ringout", "exact", "side_take", "side_yield", "side_handon", "grow_yield",
                 "grow_handon")
# the statistics counter slots of pt_selftest_ray_intersection's counters8 (csrc/device/pt_kernels.h CTR_*)
CTR_RAYS, CTR_NODES, CTR_PTESTS, CTR_PLANES, CTR_ERRORS, CTR_AUX, CTR_FALLBACKS, CTR_FALLBACKS_RAY = range(8)
ABI_VERSION = 6
# a ray query's hit record (pt_ray_hit, 24 B); a miss is id = -1 with the other fields 0
HIT_DTYPE = np.dtype([("id", np.int32), ("t", np.float32), ("n", np.float32, (3,)), ("interior", np.uint32)])
RAYS_CHUNK = 1 << 22   # pt_intersect moves the rays in chunks of at most this many
# batch radiance records (pt_path_ray 32 B, pt_path_out 16 B): one record = one RayTrace call
PATH_DTYPE = np.dtype([("o", np.float32, (3,)), ("d", np.float32, (3,)), ("seed", np.uint32), ("reserved", np.uint32)])
RADIANCE_DTYPE = np.dtype([("rgb", np.float32, (3,)), ("rays", np.uint32)])
PATHS_CHUNK = 1 << 22   # pt_radiance moves the paths in chunks of at most this many
# a pixel's sampling state (pt_pixel_state, 32 B): rng = the minstd_rand state, bit 31 set = `saved` is the
# normal_distribution's saved value; sum / samples = Scene::Sample's summary and its loop counter
PIXEL_DTYPE = np.dtype([("rng", np.uint32), ("saved", np.float32), ("x", np.uint32), ("y", np.uint32),
                        ("sum", np.float32, (3,)), ("samples", np.uint32)])
# pt_feature / pt_prim_shade (include/pt.h "first-hit features")
FEATURE_DTYPE = np.dtype([("id", np.int32), ("t", np.float32), ("n", np.float32, (3,)), ("interior", np.uint32),
                          ("albedo", np.float32, (3,)), ("ior", np.float32), ("emission", np.float32, (3,)),
                          ("material", np.uint32), ("type", np.uint32), ("reserved", np.uint32)])
SHADE_DTYPE = np.dtype([("albedo", np.float32, (3,)), ("ior", np.float32), ("emission", np.float32, (3,)),
                        ("material", np.uint32)])
FILTER_ROWMAJOR, FILTER_TILES = 0, 1   # pt_filter_opts.layout (include/pt.h "guided filter")
FEATS_CHUNK = 1 << 22    # pt_features moves the points in chunks of at most this many
PIXELS_CHUNK = 1 << 22   # pt_sample_pixels moves the records in chunks of at most this many
# pt_selftest_math's ops (include/pt.h PT_MATH_*): name -> (op, record in, record out; None = 3n f32)
_VECS = np.dtype([("v", np.float32, (8, 3))])
MATH_OPS = {
    "LOGF": (0, np.dtype(np.float32), np.dtype(np.float32)),
    "RNG": (1, np.dtype([("seed", np.uint32), ("n", np.uint32)]), None),
    "NORMAL3": (2, np.dtype([("seed", np.uint32), ("pre", np.uint32)]), _VECS),
    "COSINE": (3, np.dtype([("seed", np.uint32), ("pre", np.uint32), ("n", np.float32, (3,))]), _VECS),
    "FRESNEL": (4, np.dtype([("eta1", np.float32), ("eta2", np.float32), ("cosn", np.float32)]), np.dtype(np.float32)),
    "RESOLVE": (5, np.dtype([("sum", np.float32), ("samples", np.uint32)]),
                np.dtype([("mean", np.float32), ("byte", np.uint32)])),
    "ARITH": (6, np.dtype([("a", np.float32), ("b", np.float32), ("ad", np.float64), ("bd", np.float64)]),
              np.dtype([("quot", np.float32), ("root", np.float32), ("quotd", np.float64), ("rootd", np.float64),
                        ("narrow", np.float32), ("round_trip", np.float32)])),
}

# One HIP runtime per process: PyTorch bundles its own libamdhip64 (soname
# libamdhip64.so.7, but its users link the unversioned name), so loading
# libpt.so first would map the system copy and torch would then map a second
# runtime that cannot share the device.  Importing torch first makes libpt's
# DT_NEEDED libamdhip64.so.7 bind to torch's already-loaded runtime.
try:
    import torch  # noqa: F401
except ImportError:
    pass

if not os.path.exists(LIB_PATH):
    raise ImportError("libpt.so not built at %s (run `make -C raytracing-course_amd` or "
                      "`python -c 'import __graft_entry__ as g; g.build()'`)" % LIB_PATH)
_lib = C.CDLL(LIB_PATH)


class SceneInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "width", "height", "samples", "ray_depth", "n_prims", "n_bvh_prims", "n_planes", "n_emitters",
        "n_nodes", "tree_depth", "max_stack", "n_aux_nodes", "aux_depth", "n_warnings")]


class RenderOpts(C.Structure):
    _fields_ = [("device", C.c_int32), ("ngpu", C.c_int32), ("spp_per_launch", C.c_uint32),
                ("samples", C.c_uint32), ("traversal", C.c_int32), ("progress", C.c_int32),
                ("win_x0", C.c_uint32), ("win_y0", C.c_uint32), ("win_w", C.c_uint32), ("win_h", C.c_uint32),
                ("gather", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("node_visits", C.c_uint64), ("prim_tests", C.c_uint64),
                ("plane_tests", C.c_uint64), ("samples", C.c_uint64), ("errors", C.c_uint64),
                ("aux_visits", C.c_uint64), ("fallbacks", C.c_uint64),
                ("kernel_ms", C.c_double), ("resolve_ms", C.c_double), ("wall_ms", C.c_double),
                ("node_bytes", C.c_uint64), ("prim_bytes", C.c_uint64), ("aux_bytes", C.c_uint64),
                ("fallbacks_ray", C.c_uint64), ("isect_ms", C.c_double), ("isect_launches", C.c_uint64),
                ("rounds", C.c_uint64), ("gather_rccl", C.c_uint64),
                ("coop_rays", C.c_uint64), ("coop_node_visits", C.c_uint64), ("coop_prim_tests", C.c_uint64),
                ("coop_aux_visits", C.c_uint64), ("coop_ms", C.c_double), ("coop_launches", C.c_uint64),
                ("short_pixels", C.c_uint64), ("handed_on", C.c_uint64), ("gather_allocs", C.c_uint64),
                ("handoff", C.c_uint64 * 12)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["handoff"] = {name: int(self.handoff[i]) for i, name in enumerate(HANDOFF_SITES)}
        return d


class SessionOpts(C.Structure):
    _fields_ = [("device", C.c_int32), ("rank", C.c_uint32), ("world", C.c_uint32), ("traversal", C.c_int32),
                ("win_x0", C.c_uint32), ("win_y0", C.c_uint32), ("win_w", C.c_uint32), ("win_h", C.c_uint32)]


class RefineOpts(C.Structure):
    _fields_ = [("threshold", C.c_float), ("step", C.c_uint32), ("max_samples", C.c_uint32), ("spread", C.c_uint32)]


class RefineResult(C.Structure):
    _fields_ = [("refined", C.c_uint64), ("samples", C.c_uint64), ("unmarked", C.c_uint64), ("nonfinite", C.c_uint64),
                ("capped", C.c_uint64), ("worst", C.c_float), ("least", C.c_uint32), ("most", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FilterOpts(C.Structure):
    """pt_filter_opts; FilterOpts.default(**changes) starts from pt_filter_opts_default"""
    _fields_ = [("levels", C.c_uint32), ("sigma_c", C.c_float), ("sigma_z", C.c_float), ("sigma_a", C.c_float),
                ("normal_pow2", C.c_uint32), ("layout", C.c_uint32)]

    @classmethod
    def default(cls, **changes):
        o = cls()
        _lib.pt_filter_opts_default(C.byref(o))
        for k, v in changes.items():
            if k not in dict(cls._fields_):
                raise TypeError("no filter option %r" % k)
            setattr(o, k, v)
        return o

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_P = C.c_void_p
_sig = {
    "pt_scene_load": (C.c_int, [C.c_char_p, C.POINTER(_P)]),
    "pt_scene_load_mem": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(_P)]),
    "pt_scene_prepare": (C.c_int, [_P]),
    "pt_device_init": (C.c_int, [C.c_int]),
    "pt_gather_init": (C.c_int, [C.c_int, C.c_int]),
    "pt_scene_get_info": (C.c_int, [_P, C.POINTER(SceneInfo)]),
    "pt_scene_override": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "pt_scene_dump_bvh": (C.c_int, [_P, _P, C.c_size_t, _P, C.c_size_t]),
    "pt_scene_free": (None, [_P]),
    "pt_render_opts_default": (None, [C.POINTER(RenderOpts)]),
    "pt_render": (C.c_int, [_P, C.POINTER(RenderOpts), _P, _P, C.POINTER(Stats)]),
    "pt_write_ppm": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, _P]),
    "pt_session_create": (C.c_int, [_P, C.POINTER(SessionOpts), C.POINTER(_P)]),
    "pt_session_layout": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "pt_session_trace": (C.c_int, [_P, C.c_uint32]),
    "pt_session_resolve": (C.c_int, [_P, _P, _P]),
    "pt_session_sync": (C.c_int, [_P]),
    "pt_session_reset": (C.c_int, [_P]),
    "pt_session_read_packed": (C.c_int, [_P, _P, C.c_size_t]),
    "pt_unpack_tiles": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P]),
    "pt_unpack_tiles_f32": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P]),
    "pt_session_stats": (C.c_int, [_P, C.POINTER(Stats)]),
    "pt_session_stream": (_P, [_P]),
    "pt_session_free": (None, [_P]),
    "pt_session_pixels": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "pt_session_export": (C.c_int, [_P, _P, C.c_uint64]),
    "pt_session_import": (C.c_int, [_P, C.c_uint64, _P, C.POINTER(C.c_uint64)]),
    "pt_session_export_host": (C.c_int, [_P, _P, C.c_uint64]),
    "pt_session_import_host": (C.c_int, [_P, C.c_uint64, _P, C.POINTER(C.c_uint64)]),
    "pt_session_trace_counts": (C.c_int, [_P, C.c_uint64, _P]),
    "pt_session_trace_counts_host": (C.c_int, [_P, C.c_uint64, _P]),
    "pt_session_import_ragged": (C.c_int, [_P, C.c_uint64, _P, C.POINTER(C.c_uint64)]),
    "pt_session_import_ragged_host": (C.c_int, [_P, C.c_uint64, _P, C.POINTER(C.c_uint64)]),
    "pt_session_samples_range": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "pt_session_mark": (C.c_int, [_P]),
    "pt_session_noise": (C.c_int, [_P, _P, C.c_uint64]),
    "pt_session_noise_host": (C.c_int, [_P, _P, C.c_uint64]),
    "pt_session_plan": (C.c_int, [_P, C.POINTER(RefineOpts), _P, C.c_uint64, C.POINTER(RefineResult)]),
    "pt_session_plan_host": (C.c_int, [_P, C.POINTER(RefineOpts), _P, C.c_uint64, C.POINTER(RefineResult)]),
    "pt_session_refine": (C.c_int, [_P, C.POINTER(RefineOpts), C.POINTER(RefineResult)]),
    "pt_rayq_create": (C.c_int, [_P, C.c_int, C.c_uint64, C.POINTER(_P)]),
    "pt_rayq_run": (C.c_int, [_P, _P, C.c_uint64, _P, _P]),
    "pt_rayq_stats": (C.c_int, [_P, C.POINTER(Stats)]),
    "pt_rayq_free": (None, [_P]),
    "pt_intersect": (C.c_int, [_P, C.c_int, C.c_uint64, _P, _P, C.POINTER(Stats)]),
    "pt_pathq_create": (C.c_int, [_P, C.c_int, C.c_uint64, C.POINTER(_P)]),
    "pt_pathq_run": (C.c_int, [_P, _P, C.c_uint64, _P, _P]),
    "pt_pathq_stats": (C.c_int, [_P, C.POINTER(Stats)]),
    "pt_pathq_free": (None, [_P]),
    "pt_radiance": (C.c_int, [_P, C.c_int, C.c_uint64, _P, _P, C.POINTER(Stats)]),
    "pt_camera_rays": (C.c_int, [_P, C.c_uint64, _P, _P]),
    "pt_pixel_init": (C.c_int, [_P, C.c_uint64, _P, _P, _P]),
    "pt_pixq_create": (C.c_int, [_P, C.c_int, C.c_uint64, C.POINTER(_P)]),
    "pt_pixq_run": (C.c_int, [_P, _P, C.c_uint64, _P, _P, C.c_uint32]),
    "pt_pixq_stats": (C.c_int, [_P, C.POINTER(Stats)]),
    "pt_pixq_free": (None, [_P]),
    "pt_sample_pixels": (C.c_int, [_P, C.c_int, C.c_uint64, _P, _P, C.c_uint32, C.POINTER(Stats)]),
    "pt_pixel_resolve": (C.c_int, [_P, C.c_uint64, _P, _P, _P]),
    "pt_featq_create": (C.c_int, [_P, C.c_int, C.c_uint64, C.POINTER(_P)]),
    "pt_featq_run": (C.c_int, [_P, _P, C.c_uint64, _P, _P]),
    "pt_featq_stats": (C.c_int, [_P, C.POINTER(Stats)]),
    "pt_featq_free": (None, [_P]),
    "pt_features": (C.c_int, [_P, C.c_int, C.c_uint64, _P, _P, C.POINTER(Stats)]),
    "pt_session_features": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(Stats)]),
    "pt_session_features_host": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(Stats)]),
    "pt_scene_shade": (C.c_int, [_P, _P, C.c_size_t]),
    "pt_scene_background": (C.c_int, [_P, _P]),
    "pt_filter_opts_default": (None, [C.POINTER(FilterOpts)]),
    "pt_filtq_create": (C.c_int, [_P, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "pt_filtq_set_features": (C.c_int, [_P, _P, _P]),
    "pt_filtq_run": (C.c_int, [_P, _P, C.POINTER(FilterOpts), _P, _P, _P]),
    "pt_filtq_stats": (C.c_int, [_P, C.POINTER(Stats)]),
    "pt_filtq_free": (None, [_P]),
    "pt_filter": (C.c_int, [_P, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(FilterOpts), _P, _P,
                            _P]),
    "pt_last_error": (C.c_char_p, []),
    "pt_abi_version": (C.c_int, []),
    "pt_selftest_ray_intersection": (C.c_int, [_P, C.c_int32, C.c_uint32, _P, _P, _P, _P]),
    "pt_selftest_render_host": (C.c_int, [_P, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.c_uint32, _P]),
    "pt_selftest_paths_host": (C.c_int, [_P, C.c_uint64, _P, _P, _P]),
    "pt_selftest_pixels_host": (C.c_int, [_P, C.c_uint64, _P, _P, C.c_uint32, _P]),
    "pt_selftest_features_host": (C.c_int, [_P, C.c_uint64, _P, _P, _P]),
    "pt_selftest_filter_host": (C.c_int, [C.c_uint32, C.c_uint32, _P, C.POINTER(FilterOpts), _P, _P]),
    "pt_selftest_gamma_table": (C.c_int, [_P, _P]),
    "pt_selftest_scene_load_stretches": (C.c_int, [C.c_char_p, C.c_size_t, C.c_uint32, C.POINTER(_P), _P, C.c_uint32,
                                                   C.POINTER(C.c_uint32)]),
    "pt_selftest_scene_dump": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t), _P, C.c_size_t,
                                         C.POINTER(C.c_size_t)]),
    "pt_selftest_wave_plan": (C.c_int, [_P, C.POINTER(SessionOpts), C.c_uint32, C.c_char_p, C.c_size_t]),
    "pt_selftest_fold_shape": (C.c_int, [C.c_uint32] * 4 + [C.POINTER(C.c_uint32)] * 2),
    "pt_selftest_fit_block": (C.c_int, [C.c_uint32] * 2 + [C.POINTER(C.c_uint32)] * 3),
    "pt_selftest_lane_shape": (C.c_int, [_P] + [C.POINTER(C.c_uint32)] * 5),
    "pt_selftest_ctx_shape": (C.c_int, [C.c_uint32, _P] + [C.POINTER(C.c_uint32)] * 3),
    "pt_selftest_state_slots": (C.c_int, [_P, C.POINTER(SessionOpts), C.c_uint64, _P, _P]),
    "pt_selftest_count_records": (C.c_int, [_P, C.POINTER(SessionOpts), C.c_uint64, _P, C.POINTER(C.c_uint64)]),
    "pt_selftest_count_step": (C.c_int, [C.c_uint32, C.c_uint64, _P, _P, _P, _P, C.POINTER(C.c_uint32)]),
    "pt_selftest_refine_plan": (C.c_int, [_P, C.POINTER(SessionOpts), C.c_uint64, _P, _P, C.POINTER(RefineOpts), _P, _P,
                                          C.POINTER(RefineResult)]),
    "pt_selftest_math": (C.c_int, [C.c_int, C.c_uint32, C.c_uint64, _P, _P]),
    "pt_selftest_decide": (C.c_int, [C.c_uint64, C.c_uint64, _P]),
    "pt_selftest_decide_states": (C.c_int, [C.c_int, C.c_uint64, C.c_uint64, _P, C.c_uint64, _P,
                                            C.POINTER(C.c_uint32)]),
    "pt_selftest_aux_words": (C.c_int, [_P, _P]),
}
for _name, (_res, _args) in _sig.items():
    _f = getattr(_lib, _name)
    _f.restype = _res
    _f.argtypes = _args

EXPORTED = tuple(_sig)


class PTError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (code %d)" % (msg, code))
        self.code = code


def _check(rc):
    if rc != PT_OK:
        raise PTError(rc, _lib.pt_last_error().decode(errors="replace"))
    return rc


def last_error():
    """pt_last_error(): the message of the calling thread's last failure (also one a call
    recovered from, such as the RCCL gather's fail-over to the host)."""
    return _lib.pt_last_error().decode(errors="replace")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _counters8(ctr):
    """a host twin's counters8 (slots CTR_RAYS .. CTR_FALLBACKS_RAY), named as pt_stats names them"""
    return {"rays": int(ctr[CTR_RAYS]), "node_visits": int(ctr[CTR_NODES]), "prim_tests": int(ctr[CTR_PTESTS]),
            "plane_tests": int(ctr[CTR_PLANES]), "errors": int(ctr[CTR_ERRORS]), "aux_visits": int(ctr[CTR_AUX]),
            "fallbacks": int(ctr[CTR_FALLBACKS]), "fallbacks_ray": int(ctr[CTR_FALLBACKS_RAY])}


class Scene:
    """A loaded hw5 scene (owns the native pt_scene)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def load(cls, path):
        h = _P()
        _check(_lib.pt_scene_load(os.fsencode(path), C.byref(h)))
        return cls(h)

    @classmethod
    def loads(cls, text):
        b = text.encode() if isinstance(text, str) else bytes(text)
        h = _P()
        _check(_lib.pt_scene_load_mem(b, len(b), C.byref(h)))
        return cls(h)

    @classmethod
    def selftest_loads_stretches(cls, text, stretches):
        """pt_selftest_scene_load_stretches: (scene, [0, cuts..., len]) of `text` parsed in at most
        `stretches` stretches."""
        b = text.encode() if isinstance(text, str) else bytes(text)
        h, n = _P(), C.c_uint32(0)
        cuts = np.zeros(stretches + 1, np.uint64)
        _check(_lib.pt_selftest_scene_load_stretches(b, len(b), stretches, C.byref(h), _ptr(cuts), len(cuts), C.byref(n)))
        return cls(h), [int(c) for c in cuts[:n.value]]

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.pt_scene_free(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def prepare(self):
        _check(_lib.pt_scene_prepare(self._h))
        return self

    def override(self, width=0, height=0, samples=0, ray_depth=0):
        _check(_lib.pt_scene_override(self._h, width, height, samples, ray_depth))
        return self

    @property
    def info(self):
        i = SceneInfo()
        _check(_lib.pt_scene_get_info(self._h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in i._fields_}

    def dump_bvh(self):
        """(nodes bytes, prims bytes) in the SURVEY §8c fingerprint layout."""
        inf = self.info
        nb = np.zeros(inf["n_nodes"] * 40, np.uint8)
        pb = np.zeros(inf["n_prims"] * 52, np.uint8)
        _check(_lib.pt_scene_dump_bvh(self._h, _ptr(nb), nb.nbytes, _ptr(pb), pb.nbytes))
        return nb.tobytes(), pb.tobytes()

    def selftest_scene_dump(self):
        """pt_selftest_scene_dump: (dump bytes, warning lines) of the parse, before prepare()."""
        need, wneed = C.c_size_t(0), C.c_size_t(0)
        _check(_lib.pt_selftest_scene_dump(self._h, None, 0, C.byref(need), None, 0, C.byref(wneed)))
        out = np.zeros(need.value, np.uint8)
        warn = np.zeros(max(1, wneed.value), np.uint8)
        _check(_lib.pt_selftest_scene_dump(self._h, _ptr(out), out.nbytes, C.byref(need), _ptr(warn), wneed.value,
                                           C.byref(wneed)))
        return out.tobytes(), warn[:wneed.value].tobytes().decode("latin-1").split("\n")[:-1]

    def render(self, device=0, ngpu=1, samples=0, spp_per_launch=0, radiance=False, progress=False, window=None,
               traversal=TRAVERSAL_REPLAY, gather=GATHER_AUTO, check=True):
        """Render on the GPU(s): returns (rgb u8 HxWx3, radiance f32 HxWx3 | None, stats).
        check=False: a tripped exactness guard (stats["errors"] != 0, the render's error) does
        not raise.

        window=(x0, y0, w, h) renders only those pixels (global-index seeds kept).
        gather: GATHER_AUTO (RCCL when ngpu > 1), GATHER_RCCL (RCCL at any ngpu, an
        error if it fails), GATHER_HOST (never RCCL)."""
        inf = self.info
        w, h = (window[2], window[3]) if window else (inf["width"], inf["height"])
        rgb = np.zeros((h, w, 3), np.uint8)
        rad = np.zeros((h, w, 3), np.float32) if radiance else None
        o = RenderOpts()
        _lib.pt_render_opts_default(C.byref(o))
        o.device, o.ngpu, o.samples, o.spp_per_launch, o.progress = device, ngpu, samples, spp_per_launch, int(progress)
        o.traversal = traversal
        o.gather = gather
        if window:
            o.win_x0, o.win_y0, o.win_w, o.win_h = window
        st = Stats()
        rc = _lib.pt_render(self._h, C.byref(o), _ptr(rgb), _ptr(rad), C.byref(st))
        if check or not st.errors:
            _check(rc)
        return rgb, rad, st.as_dict()

    def intersect(self, rays, device=0):
        """Scene::RayIntersection for the caller's rays on the GPU: `rays` reshapes to (n, 6)
        float32 (origin, direction; used as given).  Returns (hits, stats): hits is an array of
        HIT_DTYPE, id = the primitive's index in the prepared order (dump_bvh's; planes at the
        end), -1 = a miss."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        hits = np.zeros(len(rays), HIT_DTYPE)
        st = Stats()
        _check(_lib.pt_intersect(self._h, device, len(rays), _ptr(rays), _ptr(hits), C.byref(st)))
        return hits, st.as_dict()

    def radiance(self, paths, device=0):
        """Scene::RayTrace for the caller's rays on the GPU: `paths` is an array of PATH_DTYPE
        (origin, direction -- used as given --, the seed of the path's fresh random stream,
        reserved = 0).  Returns (out, stats): out is an array of RADIANCE_DTYPE, rgb = the value
        RayTrace returns at the scene's RAY_DEPTH, rays = the path's RayIntersection calls."""
        paths = np.ascontiguousarray(paths, PATH_DTYPE).reshape(-1)
        out = np.zeros(len(paths), RADIANCE_DTYPE)
        st = Stats()
        _check(_lib.pt_radiance(self._h, device, len(paths), _ptr(paths), _ptr(out), C.byref(st)))
        return out, st.as_dict()

    def camera_rays(self, xy):
        """Camera::GetToRay for float pixel coordinates: `xy` reshapes to (n, 2) float32; returns
        (n, 6) float32 rays (origin, direction; the direction is not normalised)."""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        rays = np.zeros((len(xy), 6), np.float32)
        _check(_lib.pt_camera_rays(self._h, len(xy), _ptr(xy), _ptr(rays)))
        return rays

    def features(self, xy, device=0):
        """First-hit features on the GPU: `xy` reshapes to (n, 2) float32 image-plane positions in
        pixel units (used as given; outside the frame and non-finite allowed).  Returns (records,
        stats): records is an array of FEATURE_DTYPE -- the closest hit of Camera::GetToRay(x, y),
        then the hit primitive's albedo, ior, emission, material and type; a miss is id = -1 with
        emission = BG_COLOR and every other word 0."""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.zeros(len(xy), FEATURE_DTYPE)
        st = Stats()
        _check(_lib.pt_features(self._h, device, len(xy), _ptr(xy), _ptr(out), C.byref(st)))
        return out, st.as_dict()

    def filter(self, radiance, window=None, device=0, rgb=False, **opts):
        """The guided filter of a frame on the GPU (include/pt.h "guided filter"): `radiance` is the
        window's (h, w, 3) float32 -- window = (x0, y0, w, h), None: the full image -- or, with
        layout=FILTER_TILES, a world-1 session's packed radiance of it.  opts: FilterOpts' fields over
        pt_filter_opts_default.  Returns the filtered (h, w, 3) float32; with rgb=True also its 8-bit form."""
        o = FilterOpts.default(**opts)
        x0, y0, w, h = window or (0, 0, 0, 0)
        if not w:
            i = self.info
            w, h = i["width"], i["height"]
        radiance = np.ascontiguousarray(radiance, np.float32)
        need = (((w + 15) // 16) * ((h + 15) // 16) * 256 if o.layout == FILTER_TILES else w * h) * 3
        if radiance.size != need:
            raise ValueError("the frame holds %d floats, the window and layout need %d" % (radiance.size, need))
        out = np.zeros((h, w, 3), np.float32)
        img = np.zeros((h, w, 3), np.uint8) if rgb else None
        _check(_lib.pt_filter(self._h, device, x0, y0, w, h, C.byref(o), _ptr(radiance), _ptr(out), _ptr(img)))
        return (out, img) if rgb else out

    def shade(self):
        """Every primitive's albedo, ior, emission and material (an array of SHADE_DTYPE) in the
        prepared order: what the id of a hit or a feature record names.  After prepare()."""
        out = np.zeros(self.info["n_prims"], SHADE_DTYPE)
        _check(_lib.pt_scene_shade(self._h, _ptr(out), len(out)))
        return out

    @property
    def background(self):
        """the scene's BG_COLOR, 3 float32"""
        rgb = np.zeros(3, np.float32)
        _check(_lib.pt_scene_background(self._h, _ptr(rgb)))
        return rgb

    def pixel_init(self, xy, seeds=None):
        """Fresh sampling states (an array of PIXEL_DTYPE) for the pixels `xy` (reshapes to (n, 2)
        uint32: x, y): the stream std::minstd_rand(seed), sum and samples 0.  seeds=None: the
        reference's seed y * W + x."""
        xy = np.ascontiguousarray(xy, np.uint32).reshape(-1, 2)
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, np.uint32).reshape(-1)
            if len(seeds) != len(xy):
                raise ValueError("one seed per pixel")
        state = np.zeros(len(xy), PIXEL_DTYPE)
        _check(_lib.pt_pixel_init(self._h, len(xy), _ptr(xy), _ptr(seeds), _ptr(state)))
        return state

    @staticmethod
    def _pixel_args(state, counts):
        state = np.ascontiguousarray(state, PIXEL_DTYPE).reshape(-1).copy()
        if counts is not None:
            counts = np.ascontiguousarray(counts, np.uint32).reshape(-1)
            if len(counts) != len(state):
                raise ValueError("one count per state")
        return state, counts

    def sample_pixels(self, state, counts=None, spp=0, device=0):
        """Scene::Sample's loop on the GPU for the caller's pixel states: record i takes counts[i]
        more samples (counts=None: spp) on its own stream.  Returns (the states after them -- the
        argument is not changed --, stats)."""
        state, counts = self._pixel_args(state, counts)
        st = Stats()
        _check(_lib.pt_sample_pixels(self._h, device, len(state), _ptr(state), _ptr(counts), spp, C.byref(st)))
        return state, st.as_dict()

    def pixel_resolve(self, state):
        """(mean f32 (n, 3), rgb u8 (n, 3)) of the states: Sample's 1.f / samples * sum, and the
        tonemap, gamma and 8-bit step of the render's resolve."""
        state = np.ascontiguousarray(state, PIXEL_DTYPE).reshape(-1)
        mean = np.zeros((len(state), 3), np.float32)
        rgb = np.zeros((len(state), 3), np.uint8)
        _check(_lib.pt_pixel_resolve(self._h, len(state), _ptr(state), _ptr(mean), _ptr(rgb)))
        return mean, rgb

    # test hooks (host execution of the device traversal code; not a render path)
    def selftest_ray_intersection(self, rays, traversal=TRAVERSAL_REPLAY, check=True):
        """check=False: a counted error (the counters' "errors") does not raise"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        ids = np.zeros(len(rays), np.int32)
        hits = np.zeros((len(rays), 5), np.float32)
        ctr = np.zeros(8, np.uint64)
        rc = _lib.pt_selftest_ray_intersection(self._h, traversal, len(rays), _ptr(rays), _ptr(ids), _ptr(hits),
                                               _ptr(ctr))
        if check or not ctr[CTR_ERRORS]:
            _check(rc)
        return ids, hits, {"nodes": int(ctr[CTR_NODES]), "prim_tests": int(ctr[CTR_PTESTS]), "aux": int(ctr[CTR_AUX]),
                           "fallbacks": int(ctr[CTR_FALLBACKS]), "errors": int(ctr[CTR_ERRORS])}

    def selftest_paths_host(self, paths):
        """Scene.radiance's records run on the host (trace_path_with over the query state machine):
        returns (out, counters), the counters named as pt_stats names them"""
        paths = np.ascontiguousarray(paths, PATH_DTYPE).reshape(-1)
        out = np.zeros(len(paths), RADIANCE_DTYPE)
        ctr = np.zeros(8, np.uint64)
        _check(_lib.pt_selftest_paths_host(self._h, len(paths), _ptr(paths), _ptr(out), _ptr(ctr)))
        return out, _counters8(ctr)

    def selftest_pixels_host(self, state, counts=None, spp=0):
        """Scene.sample_pixels' records run on the host (camera_ray and trace_path_with over the query
        state machine): returns (states, counters), the counters named as pt_stats names them"""
        state, counts = self._pixel_args(state, counts)
        ctr = np.zeros(8, np.uint64)
        _check(_lib.pt_selftest_pixels_host(self._h, len(state), _ptr(state), _ptr(counts), spp, _ptr(ctr)))
        added = int(counts.sum(dtype=np.uint64)) if counts is not None else spp * len(state)
        return state, dict(_counters8(ctr), samples=added)

    def selftest_features(self, xy):
        """Scene.features' records computed on the host (camera_ray, the query state machine, the
        shade lookup): returns (records, counters), the counters named as pt_stats names them"""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        out = np.zeros(len(xy), FEATURE_DTYPE)
        ctr = np.zeros(8, np.uint64)
        _check(_lib.pt_selftest_features_host(self._h, len(xy), _ptr(xy), _ptr(out), _ptr(ctr)))
        return out, _counters8(ctr)

    def selftest_render_host(self, x0, y0, w, h, spp=0, traversal=TRAVERSAL_REPLAY):
        rad = np.zeros((h, w, 3), np.float32)
        _check(_lib.pt_selftest_render_host(self._h, traversal, x0, y0, w, h, spp, _ptr(rad)))
        return rad

    def wave_plan(self, cus, rank=0, world=1, traversal=TRAVERSAL_REPLAY, window=None):
        """A session's set-up on a device of `cus` compute units, computed without one: the
        wavefront pass's plan (a key per field; mix and mix_low tuples of four), n_slots,
        n_tiles_local, arena_bytes and aux_stack_words."""
        o = SessionOpts(0, rank, world, traversal, *(window or (0, 0, 0, 0)))
        buf = C.create_string_buffer(4096)
        _check(_lib.pt_selftest_wave_plan(self._h, C.byref(o), cus, buf, len(buf)))
        kv = (line.split("=") for line in buf.value.decode().splitlines())
        return {k: tuple(int(x) for x in v.split(",")) if "," in v else int(v) for k, v in kv}

    def selftest_state_slots(self, state, rank=0, world=1, traversal=TRAVERSAL_REPLAY, window=None):
        """Per record of `state` the slot of a (rank, world, window) session that Session.import_states
        would write it to, by the import kernels' own functions run on the host: >= 0 a slot, -1 a
        pixel of the image that is not that session's, -2 outside the image or a bad rng word."""
        state = np.ascontiguousarray(state, PIXEL_DTYPE).reshape(-1)
        o = SessionOpts(0, rank, world, traversal, *(window or (0, 0, 0, 0)))
        slots = np.zeros(len(state), np.int64)
        _check(_lib.pt_selftest_state_slots(self._h, C.byref(o), len(state), _ptr(state), _ptr(slots)))
        return slots

    def selftest_count_records(self, rank=0, world=1, traversal=TRAVERSAL_REPLAY, window=None):
        """Per slot of a (rank, world, window) session the record of its export -- the entry of
        Session.trace_counts' counts -- that is the slot's pixel, -1 for a padding lane, by the
        count kernels' own function run on the host."""
        o = SessionOpts(0, rank, world, traversal, *(window or (0, 0, 0, 0)))
        n = C.c_uint64()
        _lib.pt_selftest_count_records(self._h, C.byref(o), 0, None, C.byref(n))   # (the slots; refused when > 0)
        rec = np.zeros(n.value, np.int64)
        _check(_lib.pt_selftest_count_records(self._h, C.byref(o), len(rec), _ptr(rec), C.byref(n)))
        return rec

    def selftest_refine_plan(self, now, mark, threshold, step, max_samples=0, spread=0, rank=0, world=1,
                             traversal=TRAVERSAL_REPLAY, window=None):
        """Session.plan on the host for a (rank, world, window) session whose pixels hold the states
        `now` and were marked at the states `mark` (export order; a mark with samples == 0: no mark),
        by the plan kernel's own functions: returns (noise, counts, result dict)."""
        now = np.ascontiguousarray(now, PIXEL_DTYPE).reshape(-1)
        mark = np.ascontiguousarray(mark, PIXEL_DTYPE).reshape(-1)
        if len(now) != len(mark):
            raise ValueError("one mark per state")
        o = SessionOpts(0, rank, world, traversal, *(window or (0, 0, 0, 0)))
        ro, res = RefineOpts(threshold, step, max_samples, spread), RefineResult()
        noise, counts = np.zeros(len(now), np.float32), np.zeros(len(now), np.uint32)
        _check(_lib.pt_selftest_refine_plan(self._h, C.byref(o), len(now), _ptr(now), _ptr(mark), C.byref(ro),
                                            _ptr(noise), _ptr(counts), C.byref(res)))
        return noise, counts, res.as_dict()

    def gamma_table(self):
        t = np.zeros(256, np.float32)
        _check(_lib.pt_selftest_gamma_table(self._h, _ptr(t)))
        return t


class Session:
    """Tile-sharded progressive renderer on one device (include/pt.h sessions)."""

    def __init__(self, scene, device=0, rank=0, world=1, traversal=TRAVERSAL_REPLAY, window=None):
        self.scene = scene
        o = SessionOpts(device, rank, world, traversal, *(window or (0, 0, 0, 0)))
        self._h = _P()
        _check(_lib.pt_session_create(scene._h, C.byref(o), C.byref(self._h)))
        nt, nb = C.c_uint32(), C.c_uint64()
        _check(_lib.pt_session_layout(self._h, C.byref(nt), C.byref(nb)))
        self.n_tiles, self.packed_bytes = nt.value, nb.value
        self.rank, self.world = rank, world

    def trace(self, spp):
        _check(_lib.pt_session_trace(self._h, spp))

    def resolve(self, dev_out=None, dev_rad=None):
        _check(_lib.pt_session_resolve(self._h, dev_out, dev_rad))

    def sync(self):
        _check(_lib.pt_session_sync(self._h))

    def reset(self):
        """Restart every owned pixel at sample 0 (buffers and counters kept): the next
        trace(S) renders what a new session would."""
        _check(_lib.pt_session_reset(self._h))

    def read_packed(self):
        out = np.zeros(self.packed_bytes, np.uint8)
        _check(_lib.pt_session_read_packed(self._h, _ptr(out), out.nbytes))
        return out

    def stats(self):
        st = Stats()
        _check(_lib.pt_session_stats(self._h, C.byref(st)))
        return st.as_dict()

    @property
    def stream(self):
        return _lib.pt_session_stream(self._h)

    @property
    def n_pixels(self):
        """the pixels this session owns: the records of an export"""
        n = C.c_uint64()
        _check(_lib.pt_session_pixels(self._h, C.byref(n)))
        return n.value

    def export_states(self, dev=None):
        """Every owned pixel's sampling state, in slot order (rank_pixels' order): an array of
        PIXEL_DTYPE, or with `dev` -- a 16-byte aligned device address or an object with data_ptr(),
        room for n_pixels records of 32 bytes -- a fill of it (returns dev)."""
        n = self.n_pixels
        if dev is not None:
            _check(_lib.pt_session_export(self._h, _addr(dev), n))
            return dev
        state = np.zeros(n, PIXEL_DTYPE)
        _check(_lib.pt_session_export_host(self._h, _ptr(state), n))
        return state

    def import_states(self, state, n=None, ragged=False):
        """Replace the owned pixels by the caller's states: a numpy array of PIXEL_DTYPE, or a device
        address / an object with data_ptr() holding n records (n defaults to the object's size in
        bytes / 32).  Records of pixels that are not this session's are skipped; returns the number
        taken.  Every owned pixel must be named once, all at one sample count -- or, with
        ragged=True, each at its own (include/pt.h)."""
        taken = C.c_uint64()
        if isinstance(state, np.ndarray):
            state = np.ascontiguousarray(state, PIXEL_DTYPE).reshape(-1)
            f = _lib.pt_session_import_ragged_host if ragged else _lib.pt_session_import_host
            _check(f(self._h, len(state) if n is None else n, _ptr(state), C.byref(taken)))
        else:
            if n is None:
                n = state.numel() * state.element_size() // 32
            f = _lib.pt_session_import_ragged if ragged else _lib.pt_session_import
            _check(f(self._h, n, _addr(state), C.byref(taken)))
        return taken.value

    def trace_counts(self, counts, n=None):
        """Pixel i of the session, in export_states' order, takes counts[i] more samples in one pass
        of the session's engines: a numpy array of n_pixels counts, or a device address / an object
        with data_ptr() holding n uint32 (n defaults to n_pixels), which must not change before the
        next sync point.  Wavefront sessions only (include/pt.h)."""
        if isinstance(counts, np.ndarray):
            counts = np.ascontiguousarray(counts, np.uint32).reshape(-1)
            _check(_lib.pt_session_trace_counts_host(self._h, len(counts) if n is None else n, _ptr(counts)))
        else:
            _check(_lib.pt_session_trace_counts(self._h, self.n_pixels if n is None else n, _addr(counts)))

    def samples_range(self):
        """(the smallest, the largest) sample count of the session's pixels, trace() calls not yet
        run included"""
        lo, hi = C.c_uint32(), C.c_uint32()
        _check(_lib.pt_session_samples_range(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    @property
    def ragged(self):
        """whether the session's pixels hold different sample counts"""
        lo, hi = self.samples_range()
        return lo != hi

    def mark(self):
        """Remember every owned pixel's sum and count: the state its noise is measured against
        (include/pt.h "session noise").  Wavefront sessions only, as every noise call."""
        _check(_lib.pt_session_mark(self._h))

    def noise(self, dev=None):
        """Every owned pixel's noise since its mark, in export_states' order (+inf: no estimate): a
        float32 array, or with `dev` -- a device address or an object with data_ptr(), room for
        n_pixels float32 -- a fill of it (returns dev)."""
        n = self.n_pixels
        if dev is not None:
            _check(_lib.pt_session_noise(self._h, _addr(dev), n))
            return dev
        out = np.zeros(n, np.float32)
        _check(_lib.pt_session_noise_host(self._h, _ptr(out), n))
        return out

    def plan(self, threshold, step, max_samples=0, spread=0, dev=None):
        """The step refine() would take now, nothing of the session changed: (counts, result dict), the
        counts a uint32 array in export_states' order, or `dev` filled (room for n_pixels uint32)."""
        n = self.n_pixels
        o, res = RefineOpts(threshold, step, max_samples, spread), RefineResult()
        if dev is not None:
            _check(_lib.pt_session_plan(self._h, C.byref(o), _addr(dev), n, C.byref(res)))
            return dev, res.as_dict()
        counts = np.zeros(n, np.uint32)
        _check(_lib.pt_session_plan_host(self._h, C.byref(o), _ptr(counts), n, C.byref(res)))
        return counts, res.as_dict()

    def refine(self, threshold, step, max_samples=0, spread=0):
        """One adaptive step: every pixel whose noise is above the threshold (with spread=1 also its
        neighbours inside its tile) is marked and takes min(step, max_samples - its count) samples in
        one pass of the session's engines.  Returns the result dict; "refined" == 0: the frame is done."""
        o, res = RefineOpts(threshold, step, max_samples, spread), RefineResult()
        _check(_lib.pt_session_refine(self._h, C.byref(o), C.byref(res)))
        return res.as_dict()

    def features(self, dev=None, stats=False):
        """Every owned pixel's first-hit feature record, for the pixel's centre (x + 0.5, y + 0.5), in
        export_states' order (rank_pixels' order): an array of FEATURE_DTYPE, or with `dev` -- a 16-byte
        aligned device address or an object with data_ptr(), room for n_pixels records of 64 bytes -- a
        fill of it (returns dev).  Nothing of the session changes.  stats=True: returns (records, the
        call's stats dict)."""
        n = self.n_pixels
        st = Stats()
        if dev is not None:
            _check(_lib.pt_session_features(self._h, _addr(dev), n, C.byref(st)))
            return (dev, st.as_dict()) if stats else dev
        out = np.zeros(n, FEATURE_DTYPE)
        _check(_lib.pt_session_features_host(self._h, _ptr(out), n, C.byref(st)))
        return (out, st.as_dict()) if stats else out

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.pt_session_free(self._h)
            self._h = None

    __del__ = close


def _addr(x):
    """a device address: an integer, or any object with data_ptr() (a torch tensor)"""
    return C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x)


class _Query:
    """What the device contexts below share: the handle's statistics and its release.  A subclass
    names its context's pt_*_stats and pt_*_free in _stats and _free and makes self._h."""

    _stats = _free = None

    def stats(self):
        """Wait for the last run; the counters and kernel time of the runs since the last call."""
        st = Stats()
        _check(getattr(_lib, self._stats)(self._h, C.byref(st)))
        return st.as_dict()

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            getattr(_lib, self._free)(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class RayQuery(_Query):
    """Closest-hit queries for rays already on the device (include/pt.h ray queries): one
    context per scene and device, for runs of up to max_rays rays."""

    _stats, _free = "pt_rayq_stats", "pt_rayq_free"

    def __init__(self, scene, device=0, max_rays=RAYS_CHUNK):
        self.scene = scene
        self.max_rays = max_rays
        self._h = _P()
        _check(_lib.pt_rayq_create(scene._h, device, max_rays, C.byref(self._h)))

    def run(self, rays, hits, n=None, stream=None):
        """Enqueue n queries on `stream` (a hipStream_t address; None = the null stream).  rays /
        hits: device addresses, or objects with data_ptr() -- torch tensors of 6 float32 per ray
        and 24 bytes per hit (HIT_DTYPE), used in place; n defaults to the rays tensor's
        element count / 6."""
        if n is None:
            n = rays.numel() // 6
        _check(_lib.pt_rayq_run(self._h, stream, n, _addr(rays), _addr(hits)))


class FeatureQuery(_Query):
    """First-hit features for positions already on the device (include/pt.h first-hit features):
    one context per scene and device, for runs of up to max_points positions."""

    _stats, _free = "pt_featq_stats", "pt_featq_free"

    def __init__(self, scene, max_points=FEATS_CHUNK, device=0):
        self.scene = scene
        self.max_points = max_points
        self._h = _P()
        _check(_lib.pt_featq_create(scene._h, device, max_points, C.byref(self._h)))

    def run(self, d_xy, d_out, n=None, stream=None):
        """Enqueue n positions on `stream` (a hipStream_t address; None = the null stream).  d_xy /
        d_out: device addresses, or objects with data_ptr() -- torch tensors of 2 float32 per
        position and 64 bytes per record (FEATURE_DTYPE), used in place; n defaults to the
        position tensor's element count / 2."""
        if n is None:
            n = d_xy.numel() // 2
        _check(_lib.pt_featq_run(self._h, stream, n, _addr(d_xy), _addr(d_out)))


class FilterQuery(_Query):
    """The guided filter for frames already on the device (include/pt.h "guided filter"): one context
    per scene, device and window (None: the full image); it holds the window's guides."""

    _stats, _free = "pt_filtq_stats", "pt_filtq_free"

    def __init__(self, scene, window=None, device=0):
        self.scene = scene
        x0, y0, w, h = window or (0, 0, 0, 0)
        if not w:
            i = scene.info
            w, h = i["width"], i["height"]
        self.window = (x0, y0, w, h)
        self._h = _P()
        _check(_lib.pt_filtq_create(scene._h, device, x0, y0, w, h, C.byref(self._h)))

    def set_features(self, d_features, stream=None):
        """Replace the guides by ones packed from the caller's w * h FEATURE_DTYPE records on the
        device (16-byte aligned, row-major)."""
        _check(_lib.pt_filtq_set_features(self._h, stream, _addr(d_features)))

    def run(self, d_in, d_out, d_rgb=None, stream=None, **opts):
        """Enqueue one filter run on `stream` (a hipStream_t address; None = the null stream).  d_in /
        d_out / d_rgb: device addresses, or objects with data_ptr() -- the input in opts' layout, the
        (h, w, 3) float32 output and the optional (h, w, 3) uint8 one.  opts: FilterOpts' fields over
        pt_filter_opts_default, or opts=<a FilterOpts>."""
        o = opts.pop("opts", None)
        if o is None:
            o = FilterOpts.default(**opts)
        elif opts:
            raise TypeError("either opts= or single options")
        _check(_lib.pt_filtq_run(self._h, stream, C.byref(o), _addr(d_in), _addr(d_out),
                                 _addr(d_rgb) if d_rgb is not None else None))

    def stats(self):
        """Wait for the last run; kernel_ms of the runs and rays = the guide points traced since the
        last call."""
        return super().stats()


def selftest_filter_host(features, radiance, w, h, **opts):
    """FilterQuery.run's result computed on the host, for a w x h frame with the caller's FEATURE_DTYPE
    records (row-major): the filtered (h, w, 3) float32.  Needs no device and no scene."""
    o = opts.pop("opts", None) or FilterOpts.default(**opts)
    features = np.ascontiguousarray(features, FEATURE_DTYPE).reshape(-1)
    radiance = np.ascontiguousarray(radiance, np.float32)
    need = (((w + 15) // 16) * ((h + 15) // 16) * 256 if o.layout == FILTER_TILES else w * h) * 3
    if len(features) != w * h or radiance.size != need:
        raise ValueError("w * h records and the layout's floats are needed")
    out = np.zeros((h, w, 3), np.float32)
    _check(_lib.pt_selftest_filter_host(w, h, _ptr(features), C.byref(o), _ptr(radiance), _ptr(out)))
    return out


class PathQuery(_Query):
    """Radiance along paths already on the device (include/pt.h batch radiance): one context per
    scene and device, for runs of up to max_paths paths."""

    _stats, _free = "pt_pathq_stats", "pt_pathq_free"

    def __init__(self, scene, device=0, max_paths=PATHS_CHUNK):
        self.scene = scene
        self.max_paths = max_paths
        self._h = _P()
        _check(_lib.pt_pathq_create(scene._h, device, max_paths, C.byref(self._h)))

    def run(self, dev_in, dev_out, n=None, stream=None):
        """Enqueue n paths on `stream` (a hipStream_t address; None = the null stream).  dev_in /
        dev_out: 16-byte aligned device addresses, or objects with data_ptr() -- torch tensors of
        32 bytes per path (PATH_DTYPE) and 16 bytes per result (RADIANCE_DTYPE), used in place; n
        defaults to the input tensor's size in bytes / 32."""
        if n is None:
            n = dev_in.numel() * dev_in.element_size() // 32
        _check(_lib.pt_pathq_run(self._h, stream, n, _addr(dev_in), _addr(dev_out)))


class PixelQuery(_Query):
    """Further samples for pixel states already on the device (include/pt.h pixel samples): one
    context per scene and device, for runs of up to max_pixels records."""

    _stats, _free = "pt_pixq_stats", "pt_pixq_free"

    def __init__(self, scene, device=0, max_pixels=PIXELS_CHUNK):
        self.scene = scene
        self.max_pixels = max_pixels
        self._h = _P()
        _check(_lib.pt_pixq_create(scene._h, device, max_pixels, C.byref(self._h)))

    def run(self, dev_state, counts=None, spp=0, n=None, stream=None):
        """Enqueue n records on `stream` (a hipStream_t address; None = the null stream).  dev_state:
        a 16-byte aligned device address, or an object with data_ptr() -- a torch tensor of 32
        bytes per record (PIXEL_DTYPE), updated in place; counts: the same for n uint32 (int32
        tensors of non-negative values serve), or None: spp for every record; n defaults to the
        state tensor's size in bytes / 32."""
        if n is None:
            n = dev_state.numel() * dev_state.element_size() // 32
        _check(_lib.pt_pixq_run(self._h, stream, n, _addr(dev_state), None if counts is None else _addr(counts), spp))


def tile_owner(t, tiles_x, world):
    """the rank that owns window tile t (include/pt.h sessions; pt_kernels.h tile_owner)"""
    return (t % tiles_x + t // tiles_x) % world


def rank_tiles(width, height, rank, world):
    """the window tiles of `rank`, in its local (ascending) order"""
    tiles_x, tiles_y = (width + 15) // 16, (height + 15) // 16
    return [t for t in range(tiles_x * tiles_y) if tile_owner(t, tiles_x, world) == rank]


def rank_pixels(width, height, rank, world, x0=0, y0=0):
    """the (n, 2) uint32 global x, y of the pixels a session of `rank` owns in a width x height
    window at (x0, y0), in the order Session.export_states gives their records: the rank's tiles
    ascending, a tile's pixels row-major, without the pixels an edge tile lacks"""
    tiles_x = (width + 15) // 16
    out = []
    for t in rank_tiles(width, height, rank, world):
        tx, ty = 16 * (t % tiles_x), 16 * (t // tiles_x)
        ys, xs = np.mgrid[ty:min(ty + 16, height), tx:min(tx + 16, width)]
        out.append(np.stack([x0 + xs.ravel(), y0 + ys.ravel()], axis=1))
    return np.concatenate(out).astype(np.uint32) if out else np.zeros((0, 2), np.uint32)


def unpack_tiles(packed, width, height, rank, world, out=None):
    out = np.zeros((height, width, 3), np.uint8) if out is None else out
    packed = np.ascontiguousarray(packed, np.uint8)
    _check(_lib.pt_unpack_tiles(width, height, rank, world, _ptr(packed), _ptr(out)))
    return out


def unpack_tiles_f32(packed, width, height, rank, world, out=None):
    out = np.zeros((height, width, 3), np.float32) if out is None else out
    packed = np.ascontiguousarray(packed, np.float32)
    _check(_lib.pt_unpack_tiles_f32(width, height, rank, world, _ptr(packed), _ptr(out)))
    return out


def write_ppm(path, rgb):
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w, _ = rgb.shape
    _check(_lib.pt_write_ppm(os.fsencode(path), w, h, _ptr(rgb)))


def selftest_fold_shape(cus, per_cu, block, depth):
    """(block, max_grid) of a batch context with fold records (PathQuery, PixelQuery) on a device of
    `cus` compute units that hold `per_cu` workgroups of `block` threads each, at RAY_DEPTH `depth`:
    the resident grid under the fold area's 1 GiB bound.  Needs no device and no scene."""
    b, g = C.c_uint32(), C.c_uint32()
    _check(_lib.pt_selftest_fold_shape(cus, per_cu, block, depth, C.byref(b), C.byref(g)))
    return b.value, g.value


def _fit_dict(a, d, b1, b2, fits):
    return {"aux_words": a, "dfs_words": d, "block_aux_only": b1.value, "block_both": b2.value,
            "fits_aux_only": bool(fits.value & 1), "fits_both": bool(fits.value & 2)}


def selftest_fit_block(aux_words, dfs_words):
    """The batch engines' workgroup for lanes of `aux_words` aux stack words and `dfs_words` exact-DFS
    words: block_aux_only / fits_aux_only as RayQuery and FeatureQuery choose, block_both / fits_both
    as PathQuery and PixelQuery do before the fold area's bound.  Needs no device and no scene."""
    b1, b2, fits = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(_lib.pt_selftest_fit_block(aux_words, dfs_words, C.byref(b1), C.byref(b2), C.byref(fits)))
    return _fit_dict(aux_words, dfs_words, b1, b2, fits)


def selftest_lane_shape(scene):
    """selftest_fit_block for `scene`'s own stack words (returned as aux_words, dfs_words)."""
    a, d, b1, b2, fits = (C.c_uint32() for _ in range(5))
    _check(_lib.pt_selftest_lane_shape(scene._h, C.byref(a), C.byref(d), C.byref(b1), C.byref(b2), C.byref(fits)))
    return _fit_dict(a.value, d.value, b1, b2, fits)


def selftest_ctx_shape(query):
    """(block, max_grid, per_cu) of a live RayQuery, FeatureQuery, PathQuery or PixelQuery."""
    kind = {RayQuery: 0, FeatureQuery: 1, PathQuery: 2, PixelQuery: 3}[type(query)]
    b, g, p = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(_lib.pt_selftest_ctx_shape(kind, query._h, C.byref(b), C.byref(g), C.byref(p)))
    return b.value, g.value, p.value


def selftest_math(op, records, device=-1):
    """pt_selftest_math: `records` (an array of MATH_OPS[op]'s input dtype) through the device
    code's scalar functions, on `device` or (device < 0) compiled for the host.  Returns an
    array of the op's output dtype; RNG returns float32 of shape (len(records), 3 * n)."""
    code, din, dout = MATH_OPS[op]
    records = np.ascontiguousarray(records, din).reshape(-1)
    if dout is None:
        n = int(records["n"][0]) if len(records) else 0
        out = np.zeros((len(records), 3 * n), np.float32)
    else:
        out = np.zeros(len(records), dout)
    _check(_lib.pt_selftest_math(device, code, len(records), _ptr(records), _ptr(out)))
    return out


def selftest_decide(seed, n):
    """pt_selftest_decide: q_decide against the plain loop on n seeded decision states, on the
    host.  Returns {"states", "examined", "mismatches"}."""
    out = np.zeros(3, np.uint64)
    _check(_lib.pt_selftest_decide(seed, n, _ptr(out)))
    return {"states": int(out[0]), "examined": int(out[1]), "mismatches": int(out[2])}


DECIDE_EXITS = ("leaf_check", "pass_done", "another_pass", "exact")


def selftest_decide_states(seed, n, device=-1):
    """pt_selftest_decide_states: the n states of selftest_decide after the decision, by the host's
    plain loop (device < 0) or by q_decide in a kernel on `device`.  Returns (states, exits,
    slots): uint8 of shape (n, bytes per Query), the plain loop's count per exit (DECIDE_EXITS)
    and per slot the states whose last examined slot it was."""
    nb = C.c_uint32()
    _check(_lib.pt_selftest_decide_states(device, seed, 0, None, 0, None, C.byref(nb)))
    states = np.zeros((n, nb.value), np.uint8)
    unset = np.uint64(0xffffffffffffffff)
    counts = np.full(4 + 16, unset, np.uint64)   # (4 + PT_QHK are written; PT_QHK < 16)
    _check(_lib.pt_selftest_decide_states(device, seed, n, _ptr(states), states.nbytes, _ptr(counts), C.byref(nb)))
    exits = dict(zip(DECIDE_EXITS, (int(v) for v in counts[:4])))
    return states, exits, [int(v) for v in counts[4:] if v != unset]


def selftest_aux_words(scene):
    """pt_selftest_aux_words: the query blob's aux entries against the host-form array.  Returns
    {"entries", "empty", "leaf", "internal", "mismatches"}."""
    out = np.zeros(5, np.uint64)
    _check(_lib.pt_selftest_aux_words(scene._h, _ptr(out)))
    return dict(zip(("entries", "empty", "leaf", "internal", "mismatches"), (int(v) for v in out)))


def abi_version():
    return _lib.pt_abi_version()
