"""The ABI surface of the keypoint calls (include/slamfusion.h: sf_iss_params, sf_iss_stats, sf_map_iss_saliency, sf_map_iss_keypoints,
sf_cloud_iss_keypoints, sf_features_gather): declared in the header, exported by the library, wrapped by api.Map, api.Cloud,
api.Features and api.global_register.  No device call."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARATIONS = (
    r"typedef struct { double salient_radius, non_max_radius, gamma_21, gamma_32, min_lambda3; int32_t min_neighbors, profile; } sf_iss_params;",
    r"typedef struct { int64_t n_points, n_valid, n_salient, n_keypoints, max_neighbors; float saliency_ms, nms_ms; } sf_iss_stats;",
    r"void sf_iss_default_params(sf_iss_params *p);",
    r"int sf_map_iss_saliency(sf_map *m, const sf_iss_params *p, double *lambda , int32_t *n_neighbors , uint8_t *salient );",
    r"int sf_map_iss_keypoints(sf_map *m, const sf_iss_params *p, int32_t *indices , int64_t cap, int64_t *n_keypoints, uint8_t *flags , sf_iss_stats *stats);",
    r"int sf_cloud_iss_keypoints(sf_cloud *c, const sf_iss_params *p, float cell, int32_t *indices, int64_t cap, int64_t *n_keypoints, sf_iss_stats *stats);",
    r"int sf_features_gather(sf_features *src, const int32_t *rows , int64_t k, sf_features *out);",
)
SYMBOLS = ("sf_iss_default_params", "sf_map_iss_saliency", "sf_map_iss_keypoints", "sf_cloud_iss_keypoints", "sf_features_gather")


def _header():
    with open(os.path.join(ROOT, "include", "slamfusion.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_declares_the_keypoint_calls():
    text = _header()
    for decl in DECLARATIONS:
        assert re.sub(r"\s+", " ", decl) in text, decl
    # after the registration block, before the measurement switch
    assert text.index("int sf_cloud_score_poses(") < text.index("} sf_iss_params;") < text.index("int sf_features_gather(") < text.index("int sf_map_profile_launches(")


def test_library_exports_the_keypoint_calls(api):
    lib = api.load_library()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None, name


def test_structs_and_defaults(api):
    names = ["salient_radius", "non_max_radius", "gamma_21", "gamma_32", "min_lambda3", "min_neighbors", "profile"]
    assert ctypes.sizeof(api.IssParams) == 48 and [f[0] for f in api.IssParams._fields_] == names
    assert [getattr(api.IssParams, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 44]
    names = ["n_points", "n_valid", "n_salient", "n_keypoints", "max_neighbors", "saliency_ms", "nms_ms"]
    assert ctypes.sizeof(api.IssStats) == 48 and [f[0] for f in api.IssStats._fields_] == names
    assert api.IssStats.saliency_ms.offset == 40 and api.IssStats.nms_ms.offset == 44
    p = api.IssParams(1.0, 2.0, 0.5, 0.5, 3.0, 9, 1)
    api.load_library().sf_iss_default_params(ctypes.byref(p))
    assert p.as_dict() == dict(salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_lambda3=0.0, min_neighbors=5, profile=0)
    assert api.IssStats(1, 2, 3, 4, 5, 0.5, 0.25).as_dict() == dict(n_points=1, n_valid=2, n_salient=3, n_keypoints=4, max_neighbors=5, saliency_ms=0.5, nms_ms=0.25)


def test_wrappers_and_their_defaults(api):
    empty = inspect.Parameter.empty
    p = inspect.signature(api.Map.iss_keypoints).parameters
    assert list(p) == ["self", "salient_radius", "non_max_radius", "gamma_21", "gamma_32", "min_neighbors", "min_lambda3", "profile"]
    assert [v.default for v in p.values()] == [empty, empty, empty, 0.975, 0.975, 5, 0.0, False]
    p = inspect.signature(api.Cloud.iss_keypoints).parameters
    assert list(p) == ["self", "salient_radius", "non_max_radius", "gamma_21", "gamma_32", "min_neighbors", "min_lambda3", "profile", "cell"]
    assert [v.default for v in p.values()] == [empty, empty, empty, 0.975, 0.975, 5, 0.0, False, 0.0]
    p = inspect.signature(api.Map.iss_saliency).parameters
    assert list(p)[:2] == ["self", "salient_radius"] and p["gamma_21"].default == 0.975 and p["min_neighbors"].default == 5
    assert list(inspect.signature(api.Features.gather).parameters) == ["self", "indices"]
    p = inspect.signature(api.global_register).parameters
    assert list(p)[-2:] == ["src_keypoints", "dst_keypoints"] and p["src_keypoints"].default is None and p["dst_keypoints"].default is None
    assert list(p)[:5] == ["src_cloud", "src_features", "dst_cloud", "dst_features", "distance_threshold"] and list(p)[-3] == "profile"


def test_the_keyword_form(api):
    assert api._iss_params(0.6, 0.4, 0.9, 0.8, 7, 1e-6, True).as_dict() == dict(salient_radius=0.6, non_max_radius=0.4, gamma_21=0.9, gamma_32=0.8, min_lambda3=1e-6,
                                                                                 min_neighbors=7, profile=1)


def test_argument_checks_without_a_device(api):
    """What the library refuses before it touches a device: NULL handles and parameters."""
    lib = api.load_library()
    p = api._iss_params(0.6, 0.4, 0.975, 0.975, 5, 0.0, False)
    n = ctypes.c_int64(-7)
    assert lib.sf_map_iss_saliency(None, ctypes.byref(p), None, None, None) == -1                      # SF_ERR_INVALID
    assert lib.sf_map_iss_keypoints(None, ctypes.byref(p), None, ctypes.c_int64(0), ctypes.byref(n), None, None) == -1 and n.value == -7
    assert lib.sf_cloud_iss_keypoints(None, ctypes.byref(p), ctypes.c_float(0), None, ctypes.c_int64(0), ctypes.byref(n), None) == -1 and n.value == -7
    assert lib.sf_features_gather(None, None, ctypes.c_int64(0), None) == -1
    assert b"bad arguments" in lib.sf_last_error()
    lib.sf_iss_default_params(None)                                      # a no-op


def test_the_version_stays(api):
    assert api.load_library().sf_version() == 210
