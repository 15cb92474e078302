"""The ABI surface of the descriptor calls (include/slamfusion.h: sf_features, sf_fpfh_params, sf_fpfh_stats, sf_match_params,
sf_match_stats, sf_map_compute_fpfh / _spfh, sf_cloud_compute_fpfh, sf_features_match): declared in the header, exported by the
library, wrapped by api.Features, api.Map and api.Cloud.  No device call."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARATIONS = (
    r"#define SF_FPFH_DIM 33",
    r"#define SF_ORIENT_NONE 0",
    r"#define SF_ORIENT_DIRECTION 1",
    r"#define SF_ORIENT_VIEWPOINT 2",
    r"typedef struct sf_features sf_features;",
    r"typedef struct { double radius; int32_t orient, profile; double toward[3]; } sf_fpfh_params;",
    r"typedef struct { int64_t n_points, n_valid, n_featured, n_pairs, max_pairs; float spfh_ms, fpfh_ms; } sf_fpfh_stats;",
    r"typedef struct { double ratio; int32_t mutual, profile; } sf_match_params;",
    r"typedef struct { int64_t n_src, n_dst, n_src_valid, n_dst_valid, n_matched; float match_ms; int32_t pad; } sf_match_stats;",
    r"int sf_features_create(sf_ctx *ctx, sf_features **out);",
    r"void sf_features_destroy(sf_features *f);",
    r"int sf_features_size(const sf_features *f, int64_t *n);",
    r"int sf_features_upload(sf_features *f, const float *rows , const uint8_t *valid , int64_t n);",
    r"int sf_features_download(sf_features *f, float *rows , uint8_t *valid , int64_t cap, int64_t *n);",
    r"void sf_fpfh_default_params(sf_fpfh_params *p);",
    r"int sf_map_compute_fpfh(sf_map *m, const sf_fpfh_params *p, sf_features *out, sf_fpfh_stats *stats);",
    r"int sf_map_compute_spfh(sf_map *m, const sf_fpfh_params *p, uint32_t *counts , int32_t *n_pairs );",
    r"int sf_cloud_compute_fpfh(sf_cloud *c, double normal_radius, const sf_fpfh_params *p, float cell, sf_features *out, sf_fpfh_stats *stats);",
    r"int sf_features_match(sf_features *src, sf_features *dst, const sf_match_params *p, int32_t *idx , float *dist2 , float *second2 , "
    r"int32_t *pairs , int64_t cap_pairs, sf_match_stats *stats);",
)
SYMBOLS = ("sf_features_create", "sf_features_destroy", "sf_features_size", "sf_features_upload", "sf_features_download", "sf_fpfh_default_params",
           "sf_match_default_params", "sf_map_compute_fpfh", "sf_map_compute_spfh", "sf_cloud_compute_fpfh", "sf_features_match")


def _header():
    with open(os.path.join(ROOT, "include", "slamfusion.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_declares_the_descriptor_calls():
    text = _header()
    for decl in DECLARATIONS:
        assert re.sub(r"\s+", " ", decl) in text, decl
    # after the box block, before the measurement switch
    assert text.index("int sf_cloud_remove_boxes(") < text.index("#define SF_FPFH_DIM 33") < text.index("int sf_features_match(") < text.index("int sf_map_profile_launches(")


def test_library_exports_the_descriptor_calls(api):
    lib = api.load_library()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None, name


def test_structs_and_defaults(api):
    assert ctypes.sizeof(api.FpfhParams) == 40 and [f[0] for f in api.FpfhParams._fields_] == ["radius", "orient", "profile", "toward"]
    assert [getattr(api.FpfhParams, n).offset for n in ("radius", "orient", "profile", "toward")] == [0, 8, 12, 16]
    assert ctypes.sizeof(api.FpfhStats) == 48 and [f[0] for f in api.FpfhStats._fields_] == ["n_points", "n_valid", "n_featured", "n_pairs", "max_pairs", "spfh_ms", "fpfh_ms"]
    assert api.FpfhStats.spfh_ms.offset == 40 and api.FpfhStats.fpfh_ms.offset == 44
    assert ctypes.sizeof(api.MatchParams) == 16 and [f[0] for f in api.MatchParams._fields_] == ["ratio", "mutual", "profile"]
    assert ctypes.sizeof(api.MatchStats) == 48 and [f[0] for f in api.MatchStats._fields_] == ["n_src", "n_dst", "n_src_valid", "n_dst_valid", "n_matched", "match_ms", "pad"]
    assert api.MatchStats.match_ms.offset == 40
    assert api.ORIENT_MODES == dict(none=0, direction=1, viewpoint=2) and api.FPFH_DIM == 33
    lib = api.load_library()
    p = api.FpfhParams(1.0, 2, 1, (5.0, 5.0, 5.0))
    lib.sf_fpfh_default_params(ctypes.byref(p))
    assert p.as_dict() == dict(radius=0.0, orient=0, profile=0, toward=[0.0, 0.0, 1.0])
    m = api.MatchParams(0.5, 1, 1)
    lib.sf_match_default_params(ctypes.byref(m))
    assert (m.ratio, m.mutual, m.profile) == (0.0, 0, 0)
    assert api.FpfhStats(1, 2, 3, 4, 5, 0.5, 0.25).as_dict() == dict(n_points=1, n_valid=2, n_featured=3, n_pairs=4, max_pairs=5, spfh_ms=0.5, fpfh_ms=0.25)
    assert api.MatchStats(1, 2, 3, 4, 5, 0.5, 9).as_dict() == dict(n_src=1, n_dst=2, n_src_valid=3, n_dst_valid=4, n_matched=5, match_ms=0.5)


def test_wrappers_and_their_defaults(api):
    empty = inspect.Parameter.empty
    p = inspect.signature(api.Map.compute_fpfh).parameters
    assert list(p) == ["self", "radius", "orient", "toward", "profile"] and [v.default for v in p.values()] == [empty, empty, "none", (0, 0, 1), False]
    p = inspect.signature(api.Map.compute_spfh).parameters
    assert list(p) == ["self", "radius", "orient", "toward"] and [v.default for v in p.values()] == [empty, empty, "none", (0, 0, 1)]
    p = inspect.signature(api.Cloud.compute_fpfh).parameters
    assert list(p) == ["self", "normal_radius", "radius", "orient", "toward", "cell", "profile"]
    assert [v.default for v in p.values()] == [empty, empty, empty, "none", (0, 0, 1), 0.0, False]
    p = inspect.signature(api.Features.match).parameters
    assert list(p) == ["self", "other", "ratio", "mutual", "max_pairs", "profile"] and [v.default for v in p.values()] == [empty, empty, 0, False, None, False]
    assert list(inspect.signature(api.Features.upload).parameters) == ["self", "rows", "valid"]
    assert "Features" in inspect.getsource(api._close_all)               # closed before its context at exit


def test_the_keyword_form(api):
    assert api._fpfh_params(0.5, "viewpoint", (1, 2, 3), True).as_dict() == dict(radius=0.5, orient=2, profile=1, toward=[1.0, 2.0, 3.0])
    assert api._fpfh_params(2, "none", (0, 0, 1), False).as_dict() == dict(radius=2.0, orient=0, profile=0, toward=[0.0, 0.0, 1.0])
    assert api._fpfh_params(1, 7, (0, 0, 1), 0).orient == 7              # an unknown number reaches the library, which refuses it
    with pytest.raises(ValueError):
        api._fpfh_params(1, "sideways", (0, 0, 1), False)
    with pytest.raises(ValueError):
        api._fpfh_params(1, "none", (0, 0), False)


def test_argument_checks_without_a_device(api):
    """What the library refuses before it touches a device: NULL handles and parameters."""
    lib = api.load_library()
    p, mp = api.FpfhParams(0.5, 0, 0, (0.0, 0.0, 1.0)), api.MatchParams(0.0, 0, 0)
    n = ctypes.c_int64(-7)
    assert lib.sf_features_create(None, None) == -1                      # SF_ERR_INVALID
    assert lib.sf_features_size(None, ctypes.byref(n)) == -1 and n.value == -7
    assert lib.sf_features_upload(None, None, None, ctypes.c_int64(0)) == -1
    assert lib.sf_features_download(None, None, None, ctypes.c_int64(0), None) == -1
    assert lib.sf_map_compute_fpfh(None, ctypes.byref(p), None, None) == -1
    assert lib.sf_map_compute_spfh(None, ctypes.byref(p), None, None) == -1
    assert lib.sf_cloud_compute_fpfh(None, ctypes.c_double(0.5), ctypes.byref(p), ctypes.c_float(0), None, None) == -1
    assert lib.sf_features_match(None, None, ctypes.byref(mp), None, None, None, None, ctypes.c_int64(0), None) == -1
    lib.sf_features_destroy(None)                                        # a no-op
    lib.sf_fpfh_default_params(None)
    lib.sf_match_default_params(None)
    assert b"bad arguments" in lib.sf_last_error()


def test_the_version_stays(api):
    assert api.load_library().sf_version() == 210
