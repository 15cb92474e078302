"""The ABI surface of the pose-from-matches calls (include/slamfusion.h: sf_reg_params, sf_reg_candidate, sf_reg_stats,
sf_cloud_register_pairs, sf_cloud_pair_hypotheses, sf_cloud_score_poses, sf_test_score_poses): declared in the header, exported by
the library, wrapped by api.Cloud and api.global_register.  No device call."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARATIONS = (
    r"typedef struct { double distance_threshold, edge_similarity; int32_t num_hypotheses, refine_rounds; int64_t min_inliers; "
    r"int32_t top_k, profile; uint64_t seed; } sf_reg_params;",
    r"typedef struct { int32_t h, status; int64_t count; double T[16]; } sf_reg_candidate;",
    r"typedef struct { int64_t n_pairs, n_degenerate, n_rejected, n_scored, best, best_count, n_inliers; int32_t found, rounds_done; "
    r"double fitness, rmse; float hyp_ms, score_ms, refit_ms; int32_t n_top; } sf_reg_stats;",
    r"void sf_reg_default_params(sf_reg_params *p);",
    r"int sf_cloud_register_pairs(sf_cloud *src, sf_cloud *dst, const int32_t *pairs , int64_t m, const sf_reg_params *p, "
    r"double *T , uint8_t *inlier , sf_reg_candidate *top , sf_reg_stats *stats);",
    r"int sf_cloud_pair_hypotheses(sf_cloud *src, sf_cloud *dst, const int32_t *pairs , int64_t m, const sf_reg_params *p, "
    r"int32_t *samples , int32_t *status , double *T );",
    r"int sf_cloud_score_poses(sf_cloud *src, sf_cloud *dst, const int32_t *pairs , int64_t m, const float *T12 , "
    r"int64_t n_poses, double distance_threshold, int64_t *counts );",
    r"int sf_test_score_poses(sf_cloud *src, sf_cloud *dst, const int32_t *pairs, int64_t m, const float *T12, int64_t n_poses, "
    r"double distance_threshold, int max_blocks, int64_t pair_chunk, int64_t *counts);",
)
SYMBOLS = ("sf_reg_default_params", "sf_cloud_register_pairs", "sf_cloud_pair_hypotheses", "sf_cloud_score_poses", "sf_test_score_poses")


def _header():
    with open(os.path.join(ROOT, "include", "slamfusion.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_declares_the_registration_calls():
    text = _header()
    for decl in DECLARATIONS:
        assert re.sub(r"\s+", " ", decl) in text, decl
    # after the matching call, before the measurement switch; the hook beside the plane's
    assert text.index("int sf_features_match(") < text.index("} sf_reg_params;") < text.index("int sf_cloud_score_poses(") < text.index("int sf_map_profile_launches(")
    assert text.index("int sf_test_plane_score(") < text.index("int sf_test_score_poses(") < text.index("int sf_test_label_boxes(")


def test_library_exports_the_registration_calls(api):
    lib = api.load_library()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None, name


def test_structs_and_defaults(api):
    P, K, S = api.RegParams, api.RegCandidate, api.RegStats
    assert ctypes.sizeof(P) == 48
    assert [f[0] for f in P._fields_] == ["distance_threshold", "edge_similarity", "num_hypotheses", "refine_rounds", "min_inliers", "top_k", "profile", "seed"]
    assert [getattr(P, n).offset for n, _ in P._fields_] == [0, 8, 16, 20, 24, 32, 36, 40]
    assert ctypes.sizeof(K) == 144 and [(n, getattr(K, n).offset) for n, _ in K._fields_] == [("h", 0), ("status", 4), ("count", 8), ("T", 16)]
    assert ctypes.sizeof(S) == 96
    assert [f[0] for f in S._fields_] == ["n_pairs", "n_degenerate", "n_rejected", "n_scored", "best", "best_count", "n_inliers", "found", "rounds_done", "fitness",
                                         "rmse", "hyp_ms", "score_ms", "refit_ms", "n_top"]
    assert [getattr(S, n).offset for n in ("found", "rounds_done", "fitness", "rmse", "hyp_ms", "score_ms", "refit_ms", "n_top")] == [56, 60, 64, 72, 80, 84, 88, 92]
    lib = api.load_library()
    p = P(1.0, 0.5, 7, 7, 7, 7, 1, 99)
    lib.sf_reg_default_params(ctypes.byref(p))
    assert p.as_dict() == dict(distance_threshold=0.0, edge_similarity=0.9, num_hypotheses=4096, refine_rounds=2, min_inliers=3, top_k=0, profile=0, seed=0)
    q = api._reg_params(0.05, 0.8, 100, 1, 5, 4, -1, True)
    assert q.as_dict() == dict(distance_threshold=0.05, edge_similarity=0.8, num_hypotheses=100, refine_rounds=1, min_inliers=5, top_k=4, profile=1, seed=(1 << 64) - 1)
    st = S(1, 2, 3, 4, 5, 6, 7, 1, 2, 0.5, 0.25, 1.0, 2.0, 3.0, 4).as_dict()
    assert st == dict(n_pairs=1, n_degenerate=2, n_rejected=3, n_scored=4, best=5, best_count=6, n_inliers=7, found=1, rounds_done=2, fitness=0.5, rmse=0.25,
                      hyp_ms=1.0, score_ms=2.0, refit_ms=3.0, n_top=4)


def test_wrappers_and_their_defaults(api):
    empty = inspect.Parameter.empty
    p = inspect.signature(api.Cloud.register_pairs).parameters
    assert list(p) == ["self", "other", "pairs", "distance_threshold", "edge_similarity", "num_hypotheses", "refine_rounds", "min_inliers", "top_k", "seed", "profile"]
    assert [v.default for v in p.values()] == [empty, empty, empty, empty, 0.9, 4096, 2, 3, 0, 0, False]
    p = inspect.signature(api.Cloud.pair_hypotheses).parameters
    assert list(p) == ["self", "other", "pairs", "edge_similarity", "num_hypotheses", "seed"] and [v.default for v in p.values()][3:] == [0.9, 4096, 0]
    assert list(inspect.signature(api.Cloud.score_poses).parameters) == ["self", "other", "pairs", "T12", "distance_threshold"]
    p = inspect.signature(api.hook_score_poses).parameters
    assert list(p) == ["src", "dst", "pairs", "T12", "distance_threshold", "max_blocks", "pair_chunk"] and [v.default for v in p.values()][5:] == [0, 0]
    p = inspect.signature(api.global_register).parameters
    assert list(p)[:5] == ["src_cloud", "src_features", "dst_cloud", "dst_features", "distance_threshold"] and p["icp"].default is None and p["top_k"].default == 0


def test_the_terrain_generator(synth):
    assert list(inspect.signature(synth.make_terrain).parameters) == ["extent_m", "spacing", "seed"]
    a, b = synth.make_terrain(6, 0.2, 3), synth.make_terrain(6, 0.2, 3)
    assert a.dtype.name == "float32" and a.ndim == 2 and a.shape[1] == 3 and a.tobytes() == b.tobytes()
    assert a.tobytes() != synth.make_terrain(6, 0.2, 4)[:len(a)].tobytes()
    assert abs(a[:, :2]).max() <= 3.0 + 1e-6 and a[:, 2].std() > 0.1   # it has shape: not a plane


def test_argument_checks_without_a_device(api):
    """What the library refuses before it touches a device: NULL handles and parameters."""
    lib = api.load_library()
    p = api._reg_params(0.05, 0.9, 64, 2, 3, 0, 0, False)
    T, st = (ctypes.c_double * 16)(*([7.0] * 16)), api.RegStats()
    st.n_pairs = -7
    z = ctypes.c_int64(0)
    assert lib.sf_cloud_register_pairs(None, None, None, z, ctypes.byref(p), T, None, None, ctypes.byref(st)) == -1   # SF_ERR_INVALID
    assert list(T) == [7.0] * 16 and st.n_pairs == -7
    assert lib.sf_cloud_register_pairs(None, None, None, z, None, T, None, None, None) == -1
    assert lib.sf_cloud_pair_hypotheses(None, None, None, z, ctypes.byref(p), None, None, None) == -1
    assert lib.sf_cloud_score_poses(None, None, None, z, None, ctypes.c_int64(1), ctypes.c_double(0.05), None) == -1
    assert lib.sf_test_score_poses(None, None, None, z, None, ctypes.c_int64(1), ctypes.c_double(0.05), 0, z, None) == -1
    assert b"bad arguments" in lib.sf_last_error()
    for field, value in (("num_hypotheses", 0), ("num_hypotheses", (1 << 20) + 1), ("refine_rounds", -1), ("refine_rounds", 9), ("min_inliers", 2), ("top_k", -1),
                         ("top_k", 65), ("edge_similarity", 1.5), ("edge_similarity", float("nan"))):
        q = api._reg_params(0.05, 0.9, 64, 2, 3, 0, 0, False)
        setattr(q, field, value)
        assert lib.sf_cloud_register_pairs(None, None, None, z, ctypes.byref(q), T, None, None, None) == -1, field
        assert field.encode() in lib.sf_last_error(), (field, lib.sf_last_error())
    lib.sf_reg_default_params(None)                                      # a no-op


def test_the_version_stays(api):
    assert api.load_library().sf_version() == 210
