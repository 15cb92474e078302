"""The ABI surface of the NDT calls (include/slamfusion.h: sf_ndt_params, sf_ndt_result, sf_ndt_stats, sf_ndt_*): declared in the header in
their place, exported by the library, mirrored by api.NdtParams / NdtResult / NdtStats and wrapped by api.Ndt.  No device call."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARATIONS = (
    r"#define SF_NDT_DIRECT1 1",
    r"#define SF_NDT_DIRECT7 7",
    r"#define SF_NDT_FLAG_NO_OVERLAP 1",
    r"typedef struct { double resolution, outlier_ratio, step_size, transformation_epsilon, min_eig_ratio, hessian_floor; int32_t min_points, neighbours, max_iterations, profile; } sf_ndt_params;",
    r"typedef struct { double T[16], score, gradient[6], hessian[36]; int64_t n_inside, n_terms; int32_t iterations, converged, modified, flags; } sf_ndt_result;",
    r"typedef struct { int64_t n_points, n_cells, n_occupied, n_voxels; int32_t dims[3]; float build_ms, align_ms; } sf_ndt_stats;",
    r"void sf_ndt_default_params(sf_ndt_params *p);",
    r"int sf_ndt_create(sf_ctx *ctx, const sf_ndt_params *p, sf_ndt **out);",
    r"void sf_ndt_destroy(sf_ndt *ndt);",
    r"int sf_ndt_set_target_cloud(sf_ndt *ndt, sf_cloud *cloud);",
    r"int sf_ndt_set_target_map(sf_ndt *ndt, sf_map *map);",
    r"int sf_ndt_download_voxels(sf_ndt *ndt, int64_t *cell, int32_t *count, double *mean, double *cov, double *icov, int64_t cap, int64_t *n);",
    r"int sf_ndt_set_source_cloud(sf_ndt *ndt, sf_cloud *cloud);",
    r"int sf_ndt_set_source_batch(sf_ndt *ndt, const float *xyz, int64_t n_per_scan, int batch);",
    r"int sf_ndt_derivatives(sf_ndt *ndt, const double *poses, int64_t k, sf_ndt_result *out);",
    r"int sf_ndt_align(sf_ndt *ndt, const double init[16], sf_ndt_result *out, double *trace);",
    r"int sf_ndt_align_batch(sf_ndt *ndt, const double *inits, sf_ndt_result *out);",
    r"int sf_ndt_stats_read(sf_ndt *ndt, sf_ndt_stats *out);",
)
SYMBOLS = ("sf_ndt_default_params", "sf_ndt_create", "sf_ndt_destroy", "sf_ndt_set_target_cloud", "sf_ndt_set_target_map", "sf_ndt_download_voxels",
           "sf_ndt_set_source_cloud", "sf_ndt_set_source_batch", "sf_ndt_derivatives", "sf_ndt_align", "sf_ndt_align_batch", "sf_ndt_stats_read")


def _header():
    with open(os.path.join(ROOT, "include", "slamfusion.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_declares_the_ndt_calls_in_their_place():
    text = _header()
    for decl in DECLARATIONS:
        assert re.sub(r"\s+", " ", decl) in text, decl
    # after the keypoint block, before the measurement switch
    assert text.index("int sf_features_gather(") < text.index("#define SF_NDT_DIRECT1") < text.index("int sf_ndt_stats_read(") < text.index("int sf_map_profile_launches(")


def test_library_exports_the_ndt_calls(api):
    lib = api.load_library()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None, name


def test_structs_and_defaults(api):
    names = ["resolution", "outlier_ratio", "step_size", "transformation_epsilon", "min_eig_ratio", "hessian_floor", "min_points", "neighbours", "max_iterations", "profile"]
    assert ctypes.sizeof(api.NdtParams) == 64 and [f[0] for f in api.NdtParams._fields_] == names
    assert [getattr(api.NdtParams, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60]
    names = ["T", "score", "gradient", "hessian", "n_inside", "n_terms", "iterations", "converged", "modified", "flags"]
    assert ctypes.sizeof(api.NdtResult) == 504 and [f[0] for f in api.NdtResult._fields_] == names
    assert [getattr(api.NdtResult, n).offset for n in names] == [0, 128, 136, 184, 472, 480, 488, 492, 496, 500]
    names = ["n_points", "n_cells", "n_occupied", "n_voxels", "dims", "build_ms", "align_ms"]
    assert ctypes.sizeof(api.NdtStats) == 56 and [f[0] for f in api.NdtStats._fields_] == names
    assert [getattr(api.NdtStats, n).offset for n in names] == [0, 8, 16, 24, 32, 44, 48]
    p = api.NdtParams(9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9, 9, 9, 9)
    api.load_library().sf_ndt_default_params(ctypes.byref(p))
    assert p.as_dict() == dict(resolution=1.0, outlier_ratio=0.55, step_size=0.1, transformation_epsilon=1e-4, min_eig_ratio=0.01, hessian_floor=1e-6,
                               min_points=6, neighbours=7, max_iterations=30, profile=0)
    assert (api.SF_NDT_DIRECT1, api.SF_NDT_DIRECT7, api.SF_NDT_FLAG_NO_OVERLAP) == (1, 7, 1)
    r = api.NdtResult()
    r.T[5], r.score, r.hessian[7], r.n_terms, r.iterations, r.converged, r.flags = 2.0, -3.0, 4.0, 11, 5, 1, 1
    d = r.as_dict()
    assert d["T64"].shape == (4, 4) and d["T64"][1, 1] == 2.0 and d["score"] == -3.0 and d["hessian"].shape == (6, 6) and d["hessian"][1, 1] == 4.0
    assert d["gradient"].shape == (6,) and d["n_terms"] == 11 and d["iterations"] == 5 and d["converged"] is True and d["flags"] == 1 and d["modified"] == 0
    s = api.NdtStats(1, 2, 3, 4, (5, 6, 7), 0.5, 0.25)
    assert s.as_dict() == dict(n_points=1, n_cells=2, n_occupied=3, n_voxels=4, dims=(5, 6, 7), build_ms=0.5, align_ms=0.25)


def test_wrapper_signatures(api):
    empty = inspect.Parameter.empty
    p = inspect.signature(api.Ndt.__init__).parameters
    assert list(p) == ["self", "ctx", "target", "resolution", "neighbours", "outlier_ratio", "min_points", "min_eig_ratio", "step_size", "transformation_epsilon",
                       "max_iterations", "hessian_floor", "profile"]
    assert [v.default for v in p.values()] == [empty, empty, empty, empty, 7, 0.55, 6, 0.01, 0.1, 1e-4, 30, 1e-6, False]
    assert list(inspect.signature(api.Ndt.voxels).parameters) == ["self"]
    assert list(inspect.signature(api.Ndt.derivatives).parameters) == ["self", "source", "poses"]
    p = inspect.signature(api.Ndt.align).parameters
    assert list(p) == ["self", "source", "init", "trace"] and p["init"].default is None and p["trace"].default is False
    assert list(inspect.signature(api.Ndt.align_batch).parameters) == ["self", "sources", "inits"]
    assert list(inspect.signature(api.Ndt.stats).parameters) == ["self"] and list(inspect.signature(api.Ndt.close).parameters) == ["self"]


def _refused(lib, call, *args):
    assert call(*args) == -1                                   # SF_ERR_INVALID
    assert b"bad arguments" in lib.sf_last_error()


def test_argument_checks_without_a_device(api):
    """What the library refuses before it touches a device.  The parameter checks come before the context is looked at: a block of
    zeroed host memory stands in for it here and is never read (every create below is refused)."""
    lib = api.load_library()
    good = api.NdtParams()
    lib.sf_ndt_default_params(ctypes.byref(good))
    out = ctypes.c_void_p(7)
    res, st, n = api.NdtResult(), api.NdtStats(), ctypes.c_int64(-7)
    pose = (ctypes.c_double * 16)()
    _refused(lib, lib.sf_ndt_create, None, ctypes.byref(good), ctypes.byref(out))
    _refused(lib, lib.sf_ndt_create, ctypes.byref(out), None, ctypes.byref(out))
    _refused(lib, lib.sf_ndt_create, ctypes.byref(out), ctypes.byref(good), None)
    for null_handle in (lambda: lib.sf_ndt_set_target_cloud(None, None), lambda: lib.sf_ndt_set_target_map(None, None),
                        lambda: lib.sf_ndt_download_voxels(None, None, None, None, None, None, ctypes.c_int64(0), ctypes.byref(n)),
                        lambda: lib.sf_ndt_set_source_cloud(None, None), lambda: lib.sf_ndt_set_source_batch(None, None, ctypes.c_int64(0), 1),
                        lambda: lib.sf_ndt_derivatives(None, pose, ctypes.c_int64(1), ctypes.byref(res)), lambda: lib.sf_ndt_align(None, pose, ctypes.byref(res), None),
                        lambda: lib.sf_ndt_align_batch(None, pose, ctypes.byref(res)), lambda: lib.sf_ndt_stats_read(None, ctypes.byref(st))):
        _refused(lib, null_handle)
    assert n.value == -7
    stand_in = ctypes.create_string_buffer(1 << 16)
    bad = dict(resolution=(0.0, -1.0, float("inf"), float("nan")), outlier_ratio=(0.0, 1.0, -0.1, float("nan")), min_points=(2, 0, -5), neighbours=(0, 3, 27),
               max_iterations=(-1, 1025), step_size=(0.0, -0.1, float("nan")))
    for field, values in bad.items():
        for v in values:
            p = api.NdtParams()
            lib.sf_ndt_default_params(ctypes.byref(p))
            setattr(p, field, v)
            _refused(lib, lib.sf_ndt_create, stand_in, ctypes.byref(p), ctypes.byref(out))
            assert out.value == 7, (field, v)
    lib.sf_ndt_default_params(None)                            # a no-op
    lib.sf_ndt_destroy(None)


def test_the_version_stays(api):
    assert api.load_library().sf_version() == 210
