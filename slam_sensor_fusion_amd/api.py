"""ctypes binding of libslamfusion.so (include/slamfusion.h) — the product's host side.

There is no CPU fallback: if the HIP library is missing or no device is present every
entry point raises.  Nothing here imports or calls anything under oracle/.
"""
import atexit
import ctypes as C
import math
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libslamfusion.so")

SF_ICP_REF_CPP, SF_ICP_O3D_P2P, SF_ICP_P2PLANE = 0, 1, 2
SF_VOXEL_PCL, SF_VOXEL_O3D, SF_VOXEL_PCL64 = 0, 1, 2
SF_FLAG_VOXEL_OVERFLOW = 1
SF_ICP_FLAG_FEW_CORR, SF_ICP_FLAG_SINGULAR, SF_ICP_FLAG_SHARD_STALE, SF_ICP_FLAG_BARRIER_TIMEOUT = 1, 2, 4, 8
PROF_NN, PROF_REDUCE, PROF_COLLECTIVE, PROF_SOLVE, PROF_SHARD_BUILD = 0, 1, 2, 3, 4
SF_ERR_COMM = -6
MODES = {"ref_cpp": SF_ICP_REF_CPP, "o3d_p2p": SF_ICP_O3D_P2P, "p2plane": SF_ICP_P2PLANE}
ROBUST_KINDS = {"none": 0, "huber": 1, "cauchy": 2, "tukey": 3, "gm": 4}  # SF_ROBUST_*


class SlamFusionError(RuntimeError):
    pass


class IcpResult(C.Structure):
    """sf_icp_result (ICPResult of icp_point_to_point.h:28-39 plus diagnostics)."""
    _fields_ = [("T", C.c_float * 16), ("error", C.c_float), ("iterations", C.c_int32),
                ("converged", C.c_int32), ("n_corr", C.c_int32), ("n_research", C.c_int32),
                ("flags", C.c_int32), ("fitness", C.c_double), ("rmse", C.c_double),
                ("T64", C.c_double * 16)]

    def as_dict(self):
        return dict(T=np.array(self.T, dtype=np.float32).reshape(4, 4),
                    T64=np.array(self.T64, dtype=np.float64).reshape(4, 4),
                    error=float(self.error), iterations=int(self.iterations),
                    converged=bool(self.converged), n_corr=int(self.n_corr),
                    n_research=int(self.n_research), flags=int(self.flags),
                    fitness=float(self.fitness), rmse=float(self.rmse))


class IcpCacheInfo(C.Structure):
    """sf_icp_cache_info: what sf_icp_test_download_cache reads of a scan's state."""
    _fields_ = [("T", C.c_double * 16), ("motion", C.c_double), ("n", C.c_int64), ("batch", C.c_int32), ("mode", C.c_int32),
                ("cache_live", C.c_int32), ("n_research", C.c_int32), ("iterations", C.c_int32), ("ordered", C.c_int32)]


COV_FLAGS = {"few_corr": 1, "singular": 2, "degenerate_trans": 4, "degenerate_rot": 8}  # SF_COV_*


class IcpCovariance(C.Structure):
    """sf_icp_covariance: pose covariance and degeneracy of one alignment, order (wx wy wz tx ty tz), T' = Exp(w, t) T."""
    _fields_ = [("info", C.c_double * 36), ("cov", C.c_double * 36), ("sigma2", C.c_double), ("sigma2_hat", C.c_double),
                ("weight_sum", C.c_double), ("trans_info", C.c_double * 3), ("trans_dir", C.c_double * 9),
                ("rot_info", C.c_double * 3), ("rot_dir", C.c_double * 9), ("n_corr", C.c_int64), ("flags", C.c_int32)]

    def as_dict(self):
        a = lambda f, *shape: np.array(f, dtype=np.float64).reshape(shape)
        return dict(info=a(self.info, 6, 6), cov=a(self.cov, 6, 6), sigma2=float(self.sigma2), sigma2_hat=float(self.sigma2_hat),
                    weight_sum=float(self.weight_sum), trans_info=a(self.trans_info, 3), trans_dir=a(self.trans_dir, 3, 3),
                    rot_info=a(self.rot_info, 3), rot_dir=a(self.rot_dir, 3, 3), n_corr=int(self.n_corr), flags=int(self.flags))


SOR_FLAVOURS = {"pcl": 0, "o3d": 1}  # SF_SOR_*


def _sor_flavour(flavour):
    return SOR_FLAVOURS[flavour] if flavour in SOR_FLAVOURS else int(flavour)


class OutlierStats(C.Structure):
    """sf_outlier_stats: what an outlier filter saw (the radius filter leaves the three doubles 0)."""
    _fields_ = [("n_points", C.c_int64), ("n_valid", C.c_int64), ("n_kept", C.c_int64), ("mean", C.c_double), ("stddev", C.c_double), ("threshold", C.c_double)]

    def as_dict(self):
        return dict(n_points=int(self.n_points), n_valid=int(self.n_valid), n_kept=int(self.n_kept), mean=float(self.mean), stddev=float(self.stddev),
                    threshold=float(self.threshold))


SF_KNN_MAX = 64
RADIUS_ORDERS = {"index": 0, "distance": 1}  # SF_RADIUS_ORDER_*
RADIUS_FILLS = {"auto": 0, "lane": 1, "wave": 2}


def _radius_order(order):
    return RADIUS_ORDERS[order] if order in RADIUS_ORDERS else int(order)


class RadiusStats(C.Structure):
    """sf_radius_stats: the rows of a radius call, those searched, those left empty, the entries in all and the longest row."""
    _fields_ = [("n_queries", C.c_int64), ("n_searched", C.c_int64), ("n_empty", C.c_int64), ("total", C.c_int64), ("max_count", C.c_int64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class ClusterStats(C.Structure):
    """sf_cluster_stats: what a clustering call found (n_noise, n_kept: the indexed points labelled -1 / the points with a label)."""
    _fields_ = [(name, C.c_int64) for name in ("n_points", "n_valid", "n_core", "n_border", "n_noise", "n_clusters", "largest_size", "n_kept")]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class PlaneParams(C.Structure):
    """sf_plane_params: what a plane segmentation is asked for (sf_plane_default_params: 0.1 m, 1024 hypotheses, refine, seed 0,
    min_inliers 3, no axis)."""
    _fields_ = [("distance_threshold", C.c_double), ("num_hypotheses", C.c_int32), ("refine", C.c_int32), ("seed", C.c_uint64), ("min_inliers", C.c_int64),
                ("axis", C.c_double * 3), ("axis_min_cos", C.c_double), ("profile", C.c_int32), ("pad", C.c_int32)]

    def as_dict(self):
        return dict(distance_threshold=float(self.distance_threshold), num_hypotheses=int(self.num_hypotheses), refine=int(self.refine), seed=int(self.seed),
                    min_inliers=int(self.min_inliers), axis=[float(v) for v in self.axis], axis_min_cos=float(self.axis_min_cos), profile=int(self.profile))


class PlaneStats(C.Structure):
    """sf_plane_stats: what a plane segmentation found (best_index / best_count: the winning hypothesis and its inliers; n_inliers:
    those of the final plane; score_ms / total_ms: -1 unless profiled)."""
    _fields_ = [(name, C.c_int64) for name in ("n_points", "n_hypotheses", "n_degenerate", "best_index", "best_count", "n_inliers")] + \
               [("found", C.c_int32), ("refined", C.c_int32), ("score_ms", C.c_float), ("total_ms", C.c_float)]

    def as_dict(self):
        return {name: (float if kind is C.c_float else int)(getattr(self, name)) for name, kind in self._fields_}


def _plane_params(distance_threshold, num_hypotheses, refine, seed, min_inliers, axis, max_angle_deg, profile):
    """The keyword form of the plane calls -> PlaneParams.  The ABI takes the cosine of the angle: it is math.cos's here."""
    p = PlaneParams()
    load_library().sf_plane_default_params(C.byref(p))
    p.distance_threshold, p.num_hypotheses, p.refine = float(distance_threshold), int(num_hypotheses), int(bool(refine))
    p.seed, p.min_inliers, p.profile = int(seed) & 0xFFFFFFFFFFFFFFFF, int(min_inliers), int(bool(profile))
    if axis is not None:
        a = [float(v) for v in np.asarray(axis, dtype=np.float64).reshape(3)]
        p.axis[0], p.axis[1], p.axis[2] = a
        p.axis_min_cos = 0.0 if max_angle_deg is None else math.cos(math.radians(float(max_angle_deg)))
    elif max_angle_deg is not None:
        raise SlamFusionError("max_angle_deg needs an axis")
    return p


BOX_MODES = {"aabb": 0, "pca": 1, "upright": 2}  # SF_BOX_*


class BoxParams(C.Structure):
    """sf_box_params: the axes rule of the per-label boxes (mode: SF_BOX_*; up: all zeros = +z) and the profile switch."""
    _fields_ = [("mode", C.c_int32), ("profile", C.c_int32), ("up", C.c_double * 3)]

    def as_dict(self):
        return dict(mode=int(self.mode), profile=int(self.profile), up=[float(v) for v in self.up])


class LabelBox(C.Structure):
    """sf_label_box (256 bytes): one label's members summed up.  center, R (row-major, columns = axes) and extent (full lengths) are
    the arguments of Cloud.crop_obb; valid: 0 no member, 1, 2 = the covariance was not finite (identity axes)."""
    _fields_ = [("count", C.c_int64), ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("mean", C.c_double * 3), ("cov", C.c_double * 6),
                ("center", C.c_double * 3), ("R", C.c_double * 9), ("extent", C.c_double * 3), ("eigenvalues", C.c_double * 3), ("valid", C.c_int32),
                ("pad", C.c_int32)]


LABEL_BOX_DTYPE = np.dtype([("count", "<i8"), ("lo", "<f4", (3,)), ("hi", "<f4", (3,)), ("mean", "<f8", (3,)), ("cov", "<f8", (6,)), ("center", "<f8", (3,)),
                            ("R", "<f8", (3, 3)), ("extent", "<f8", (3,)), ("eigenvalues", "<f8", (3,)), ("valid", "<i4"), ("pad", "<i4")])


class BoxStats(C.Structure):
    """sf_box_stats: what a box call saw (n_points = n_labelled + n_ignored + n_nonfinite; n_valid: the labels with members;
    device_ms: -1 unless profiled)."""
    _fields_ = [(name, C.c_int64) for name in ("n_points", "n_labelled", "n_ignored", "n_nonfinite", "n_labels", "n_valid")] + \
               [("device_ms", C.c_float), ("pad", C.c_int32)]

    def as_dict(self):
        return {name: (float if kind is C.c_float else int)(getattr(self, name)) for name, kind in self._fields_ if name != "pad"}


def _box_params(mode, up, profile):
    """The keyword form of the box calls -> BoxParams (mode: "aabb" | "pca" | "upright" or the SF_BOX_* number)."""
    p = BoxParams()
    p.mode, p.profile = (BOX_MODES[mode] if mode in BOX_MODES else int(mode)), int(bool(profile))
    if up is not None:
        p.up[0], p.up[1], p.up[2] = [float(v) for v in np.asarray(up, dtype=np.float64).reshape(3)]
    return p


VIS_CLASSES = dict(outside=0, unknown=1, within=2, occluded=3, seen_through=4)  # SF_VIS_*


class RangeImageParams(C.Structure):
    """sf_range_image_params: width x height pixels over the full turn of azimuth and [el_min, el_max) of elevation (radians), and
    the ranges (metres) a point must lie in to be projected."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("el_min", C.c_double), ("el_max", C.c_double), ("min_range", C.c_double), ("max_range", C.c_double)]

    def as_dict(self):
        return {name: (float if kind is C.c_double else int)(getattr(self, name)) for name, kind in self._fields_}


class RangeImageStats(C.Structure):
    """sf_range_image_stats: what a build saw (n_points = n_projected + n_outside + n_nonfinite; n_filled: the pixels that are not
    empty; device_ms: the fill and the two kernels)."""
    _fields_ = [(name, C.c_int64) for name in ("n_points", "n_projected", "n_outside", "n_nonfinite", "n_filled")] + [("device_ms", C.c_float), ("pad", C.c_int32)]

    def as_dict(self):
        return {name: (float if kind is C.c_float else int)(getattr(self, name)) for name, kind in self._fields_ if name != "pad"}


class VisibilityParams(C.Structure):
    """sf_visibility_params: the window (half_cols, half_rows pixels either side), the non-empty pixels it must hold for a verdict
    (min_hits), the profile switch, and margin = range_margin + range_ratio * r."""
    _fields_ = [("half_cols", C.c_int32), ("half_rows", C.c_int32), ("min_hits", C.c_int32), ("profile", C.c_int32), ("range_margin", C.c_double),
                ("range_ratio", C.c_double)]

    def as_dict(self):
        return {name: (float if kind is C.c_double else int)(getattr(self, name)) for name, kind in self._fields_}


class VisibilityStats(C.Structure):
    """sf_visibility_stats: the class counts summed over the images, the points and the indexed (map) or finite (cloud) ones, the
    points a cloud call took away; device_ms: -1 unless profiled."""
    _fields_ = [(name, C.c_int64) for name in ("n_points", "n_valid", "n_outside", "n_unknown", "n_within", "n_occluded", "n_seen_through", "n_removed")] + \
               [("device_ms", C.c_float), ("pad", C.c_int32)]

    def as_dict(self):
        return {name: (float if kind is C.c_float else int)(getattr(self, name)) for name, kind in self._fields_ if name != "pad"}


def _visibility_params(half_cols, half_rows, min_hits, range_margin, range_ratio, profile):
    """The keyword form of the visibility calls -> VisibilityParams."""
    return VisibilityParams(int(half_cols), int(half_rows), int(min_hits), int(bool(profile)), float(range_margin), float(range_ratio))


def _images_and_poses(images, poses):
    """-> (the array of sf_range_image handles, float64 [B, 16] or None, B)"""
    images = list(images)
    handles = (C.c_void_p * max(len(images), 1))(*[im.h for im in images])
    if poses is None:
        return handles, None, len(images)
    poses = _f64(poses).reshape(-1, 16)
    if len(poses) != len(images):
        raise SlamFusionError("one pose per image (%d images, %d poses)" % (len(images), len(poses)))
    return handles, poses, len(images)


class ScanContextParams(C.Structure):
    """sf_place_params: num_rings x num_sectors bins over [0, max_range) of horizontal range and the full turn of azimuth; a point
    nearer than min_range is left out; sensor_height is added to z so that heights count from the ground."""
    _fields_ = [("num_rings", C.c_int32), ("num_sectors", C.c_int32), ("min_range", C.c_double), ("max_range", C.c_double), ("sensor_height", C.c_double)]

    def as_dict(self):
        return {name: (float if kind is C.c_double else int)(getattr(self, name)) for name, kind in self._fields_}


class ScanContextStats(C.Structure):
    """sf_place_stats: what a descriptor build saw (n_points = n_nonfinite + n_outside + n_below + n_binned; n_filled: the bins that
    are not empty; device_ms: the fill and the two kernels)."""
    _fields_ = [(name, C.c_int64) for name in ("n_points", "n_nonfinite", "n_outside", "n_below", "n_binned", "n_filled")] + [("device_ms", C.c_float), ("pad", C.c_int32)]

    def as_dict(self):
        return {name: (float if kind is C.c_float else int)(getattr(self, name)) for name, kind in self._fields_ if name != "pad"}


class PlaceMatchStats(C.Structure):
    """sf_place_match_stats: the pairs of a call and the device time of its match and of its selection."""
    _fields_ = [("n_queries", C.c_int64), ("n_entries", C.c_int64), ("match_ms", C.c_float), ("select_ms", C.c_float)]

    def as_dict(self):
        return {name: (float if kind is C.c_float else int)(getattr(self, name)) for name, kind in self._fields_}


def _scan_context_params(num_rings=20, num_sectors=60, min_range=0.5, max_range=80.0, sensor_height=2.0):
    """The keyword form of the Scan Context calls -> ScanContextParams."""
    return ScanContextParams(int(num_rings), int(num_sectors), float(min_range), float(max_range), float(sensor_height))


ORIENT_MODES = {"none": 0, "direction": 1, "viewpoint": 2}  # SF_ORIENT_*
FPFH_DIM = 33                                               # SF_FPFH_DIM


class FpfhParams(C.Structure):
    """sf_fpfh_params: the feature radius, how the stored normals are oriented as they are loaded (SF_ORIENT_*; toward: a direction or
    a viewpoint) and the profile switch."""
    _fields_ = [("radius", C.c_double), ("orient", C.c_int32), ("profile", C.c_int32), ("toward", C.c_double * 3)]

    def as_dict(self):
        return dict(radius=float(self.radius), orient=int(self.orient), profile=int(self.profile), toward=[float(v) for v in self.toward])


class FpfhStats(C.Structure):
    """sf_fpfh_stats: n_valid = the indexed points, n_featured = the rows with a descriptor, n_pairs / max_pairs = the sum and the
    largest of the pair counts P_i; spfh_ms / fpfh_ms: -1 unless profiled."""
    _fields_ = [(name, C.c_int64) for name in ("n_points", "n_valid", "n_featured", "n_pairs", "max_pairs")] + [("spfh_ms", C.c_float), ("fpfh_ms", C.c_float)]

    def as_dict(self):
        return {name: (float if kind is C.c_float else int)(getattr(self, name)) for name, kind in self._fields_}


class MatchParams(C.Structure):
    """sf_match_params: ratio (<= 0 or >= 1: no ratio test), mutual, profile."""
    _fields_ = [("ratio", C.c_double), ("mutual", C.c_int32), ("profile", C.c_int32)]


class MatchStats(C.Structure):
    """sf_match_stats: the rows and the valid rows of both sides, the accepted pairs; match_ms: -1 unless profiled."""
    _fields_ = [(name, C.c_int64) for name in ("n_src", "n_dst", "n_src_valid", "n_dst_valid", "n_matched")] + [("match_ms", C.c_float), ("pad", C.c_int32)]

    def as_dict(self):
        return {name: (float if kind is C.c_float else int)(getattr(self, name)) for name, kind in self._fields_ if name != "pad"}


def _fpfh_params(radius, orient, toward, profile):
    """The keyword form of the FPFH calls -> FpfhParams (orient: "none" | "direction" | "viewpoint" or the SF_ORIENT_* number)."""
    p = FpfhParams()
    p.radius, p.orient, p.profile = float(radius), (ORIENT_MODES[orient] if orient in ORIENT_MODES else int(orient)), int(bool(profile))
    p.toward[0], p.toward[1], p.toward[2] = [float(v) for v in np.asarray(toward, dtype=np.float64).reshape(3)]
    return p


class RegParams(C.Structure):
    """sf_reg_params: what a pose estimation from matches is asked for (sf_reg_default_params: threshold to be set, edge similarity 0.9,
    4096 hypotheses, 2 refit rounds, min_inliers 3, top_k 0, seed 0)."""
    _fields_ = [("distance_threshold", C.c_double), ("edge_similarity", C.c_double), ("num_hypotheses", C.c_int32), ("refine_rounds", C.c_int32),
                ("min_inliers", C.c_int64), ("top_k", C.c_int32), ("profile", C.c_int32), ("seed", C.c_uint64)]

    def as_dict(self):
        return dict(distance_threshold=float(self.distance_threshold), edge_similarity=float(self.edge_similarity), num_hypotheses=int(self.num_hypotheses),
                    refine_rounds=int(self.refine_rounds), min_inliers=int(self.min_inliers), top_k=int(self.top_k), profile=int(self.profile), seed=int(self.seed))


class RegCandidate(C.Structure):
    """sf_reg_candidate (144 bytes): one of the best hypotheses -- its index, status (always 0), inlier count and transform."""
    _fields_ = [("h", C.c_int32), ("status", C.c_int32), ("count", C.c_int64), ("T", C.c_double * 16)]

    def as_dict(self):
        return dict(h=int(self.h), status=int(self.status), count=int(self.count), T=np.array(self.T, dtype=np.float64).reshape(4, 4))


class RegStats(C.Structure):
    """sf_reg_stats: n_scored = the hypotheses that were neither degenerate nor rejected; best / best_count: the winning hypothesis and
    its inliers; n_inliers, fitness, rmse: those of the final transform; n_top: the candidates returned; the times: -1 unless profiled."""
    _fields_ = [(name, C.c_int64) for name in ("n_pairs", "n_degenerate", "n_rejected", "n_scored", "best", "best_count", "n_inliers")] + \
               [("found", C.c_int32), ("rounds_done", C.c_int32), ("fitness", C.c_double), ("rmse", C.c_double), ("hyp_ms", C.c_float), ("score_ms", C.c_float),
                ("refit_ms", C.c_float), ("n_top", C.c_int32)]

    def as_dict(self):
        return {name: (int if kind in (C.c_int64, C.c_int32) else float)(getattr(self, name)) for name, kind in self._fields_}


def _reg_params(distance_threshold, edge_similarity, num_hypotheses, refine_rounds, min_inliers, top_k, seed, profile):
    """The keyword form of the registration calls -> RegParams."""
    p = RegParams()
    load_library().sf_reg_default_params(C.byref(p))
    p.distance_threshold, p.edge_similarity, p.num_hypotheses = float(distance_threshold), float(edge_similarity), int(num_hypotheses)
    p.refine_rounds, p.min_inliers, p.top_k = int(refine_rounds), int(min_inliers), int(top_k)
    p.seed, p.profile = int(seed) & 0xFFFFFFFFFFFFFFFF, int(bool(profile))
    return p


def _pairs(pairs):
    return np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)


class IssParams(C.Structure):
    """sf_iss_params: the two radii, the two eigenvalue ratios, the absolute floor of lambda3 (m^2), the least neighbour count and the
    profile switch (sf_iss_default_params: radii to be set, gammas 0.975, no floor, 5 neighbours)."""
    _fields_ = [(name, C.c_double) for name in ("salient_radius", "non_max_radius", "gamma_21", "gamma_32", "min_lambda3")] + \
               [("min_neighbors", C.c_int32), ("profile", C.c_int32)]

    def as_dict(self):
        return {name: (float if kind is C.c_double else int)(getattr(self, name)) for name, kind in self._fields_}


class IssStats(C.Structure):
    """sf_iss_stats: n_valid = the indexed points, n_salient, n_keypoints, max_neighbors = the largest count at the salient radius;
    saliency_ms / nms_ms: -1 unless profiled."""
    _fields_ = [(name, C.c_int64) for name in ("n_points", "n_valid", "n_salient", "n_keypoints", "max_neighbors")] + \
               [("saliency_ms", C.c_float), ("nms_ms", C.c_float)]

    def as_dict(self):
        return {name: (float if kind is C.c_float else int)(getattr(self, name)) for name, kind in self._fields_}


def _iss_params(salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors, min_lambda3, profile):
    """The keyword form of the ISS calls -> IssParams."""
    p = IssParams()
    load_library().sf_iss_default_params(C.byref(p))
    p.salient_radius, p.non_max_radius, p.gamma_21, p.gamma_32 = float(salient_radius), float(non_max_radius), float(gamma_21), float(gamma_32)
    p.min_lambda3, p.min_neighbors, p.profile = float(min_lambda3), int(min_neighbors), int(bool(profile))
    return p


SF_NDT_DIRECT1, SF_NDT_DIRECT7 = 1, 7
SF_NDT_FLAG_NO_OVERLAP = 1
SF_NDT_FLAG_LINE_SEARCH_STALLED = 2
SF_NDT_MAX_TRIALS = 16


class NdtParams(C.Structure):
    """sf_ndt_params (sf_ndt_default_params: resolution 1, outlier_ratio 0.55, step_size 0.1, transformation_epsilon 1e-4,
    min_eig_ratio 0.01, hessian_floor 1e-6, min_points 6, DIRECT7, 30 iterations, no profile)."""
    _fields_ = [(name, C.c_double) for name in ("resolution", "outlier_ratio", "step_size", "transformation_epsilon", "min_eig_ratio", "hessian_floor")] + \
               [(name, C.c_int32) for name in ("min_points", "neighbours", "max_iterations", "profile")]

    def as_dict(self):
        return {name: (float if kind is C.c_double else int)(getattr(self, name)) for name, kind in self._fields_}


class NdtResult(C.Structure):
    """sf_ndt_result: the pose, the NDT score with its gradient and full Hessian at that pose (order rx ry rz tx ty tz), the points
    that met a voxel, the terms, and how the alignment went."""
    _fields_ = [("T", C.c_double * 16), ("score", C.c_double), ("gradient", C.c_double * 6), ("hessian", C.c_double * 36),
                ("n_inside", C.c_int64), ("n_terms", C.c_int64), ("iterations", C.c_int32), ("converged", C.c_int32),
                ("modified", C.c_int32), ("flags", C.c_int32)]

    def as_dict(self):
        a = lambda f, *shape: np.array(f, dtype=np.float64).reshape(shape)
        return dict(T64=a(self.T, 4, 4), score=float(self.score), gradient=a(self.gradient, 6), hessian=a(self.hessian, 6, 6),
                    n_inside=int(self.n_inside), n_terms=int(self.n_terms), iterations=int(self.iterations),
                    converged=bool(self.converged), modified=int(self.modified), flags=int(self.flags))


class NdtStats(C.Structure):
    """sf_ndt_stats: the target's points, the cells of its index at `resolution`, the occupied ones, the voxels; build_ms /
    align_ms: -1 unless profiled."""
    _fields_ = [(name, C.c_int64) for name in ("n_points", "n_cells", "n_occupied", "n_voxels")] + \
               [("dims", C.c_int32 * 3), ("build_ms", C.c_float), ("align_ms", C.c_float)]

    def as_dict(self):
        return dict(n_points=int(self.n_points), n_cells=int(self.n_cells), n_occupied=int(self.n_occupied), n_voxels=int(self.n_voxels),
                    dims=tuple(int(v) for v in self.dims), build_ms=float(self.build_ms), align_ms=float(self.align_ms))


class NdtLineSearch(C.Structure):
    """sf_ndt_line_search (sf_ndt_default_line_search: 8 trials, step_max 1.0, armijo 1e-4; trials 0: off)."""
    _fields_ = [("trials", C.c_int32), ("pad", C.c_int32), ("step_max", C.c_double), ("armijo", C.c_double)]

    def as_dict(self):
        return dict(trials=int(self.trials), step_max=float(self.step_max), armijo=float(self.armijo))


class NdtLsRow(C.Structure):
    """sf_ndt_ls_row: one iteration of the line search of entry 0 -- the range, the unscaled direction `delta`, the score phi0 and the
    slope at the pose, phi / n_terms of the trials alpha_max / 2^k, and the accepted k (-1: stalled)."""
    _fields_ = [("alpha_max", C.c_double), ("raw_length", C.c_double), ("phi0", C.c_double), ("slope", C.c_double), ("delta", C.c_double * 6),
                ("phi", C.c_double * 16), ("n_terms", C.c_int64 * 16), ("chosen", C.c_int32), ("trials", C.c_int32)]

    def as_dict(self):
        k = int(self.trials)
        return dict(alpha_max=float(self.alpha_max), raw_length=float(self.raw_length), phi0=float(self.phi0), slope=float(self.slope),
                    delta=np.array(self.delta, dtype=np.float64), phi=np.array(self.phi, dtype=np.float64)[:k], n_terms=np.array(self.n_terms, dtype=np.int64)[:k],
                    chosen=int(self.chosen), trials=k)


def _rows(indices):
    return np.ascontiguousarray(np.asarray(indices).reshape(-1), dtype=np.int32)


_lib = None
_live = weakref.WeakSet()   # every wrapper object, closed in dependency order at exit


def _close_all():
    for kind in ("Node", "Comm", "Icp", "NdtPyramid", "Ndt", "BruteForceAlignment", "Features", "RangeImage", "PlaceDB", "Map", "Cloud", "Context"):
        for obj in [o for o in list(_live) if type(o).__name__ == kind]:
            try:
                obj.close()
            except Exception:
                pass


atexit.register(_close_all)


def load_library():
    """Load libslamfusion.so; fails loudly (no fallback) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SlamFusionError(
            "libslamfusion.so not found at %s — build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
            "There is no CPU fallback." % LIB_PATH)
    # This image carries two HIP runtimes (ROCm 7.2 under /opt/rocm, and the 7.0 one bundled
    # in the torch wheel).  A process must use exactly one: import torch FIRST so that the
    # library's libamdhip64.so.7 dependency resolves to the runtime torch already loaded
    # (the other order leaves torch with "No HIP GPUs are available").  torch is plumbing
    # only (streams, RCCL); nothing in the data path goes through it.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    lib.sf_last_error.restype = C.c_char_p
    lib.sf_ctx_stream.restype = C.c_void_p
    lib.sf_cloud_device_ptr.restype = C.c_void_p
    lib.sf_icp_exchange_ptr.restype = C.c_void_p
    lib.sf_sfilter_create.restype = C.c_void_p
    lib.sf_node_icp.restype = C.c_void_p
    lib.sf_node_bf.restype = C.c_void_p
    lib.sf_fusion_compass_to_yaw.restype = C.c_float
    lib.sf_fusion_closest_altitude.restype = C.c_float
    lib.sf_sfilter_pose_zscore.restype = C.c_float
    lib.sf_icp_set_robust_kernel.argtypes = [C.c_void_p, C.c_int, C.c_double]
    lib.sf_icp_set_covariance.argtypes = [C.c_void_p, C.c_int, C.c_double]
    lib.sf_icp_set_degeneracy_thresholds.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double]
    lib.sf_icp_fetch_covariance.argtypes = [C.c_void_p, C.c_void_p]
    lib.sf_icp_fetch_covariance_previous.argtypes = [C.c_void_p, C.c_void_p]
    lib.sf_test_radix_sort.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_test_scan_u32.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    lib.sf_test_linalg.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int]
    lib.sf_test_wave_reduce.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.sf_test_block_reduce.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.sf_test_reduce_partials.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.sf_plane_default_params.restype = None
    lib.sf_cloud_plane_hypotheses.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_cloud_score_planes.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p]
    lib.sf_cloud_segment_plane.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_cloud_remove_plane.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.sf_test_plane_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int, C.c_void_p]
    lib.sf_cloud_label_boxes.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_test_label_boxes.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.sf_cloud_cluster_boxes.argtypes = [C.c_void_p, C.c_double, C.c_int64, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.sf_cloud_remove_boxes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int, C.c_void_p]
    lib.sf_fpfh_default_params.restype = None
    lib.sf_match_default_params.restype = None
    lib.sf_features_create.argtypes = [C.c_void_p, C.c_void_p]
    lib.sf_features_destroy.argtypes = [C.c_void_p]
    lib.sf_features_destroy.restype = None
    lib.sf_features_size.argtypes = [C.c_void_p, C.c_void_p]
    lib.sf_features_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.sf_features_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.sf_map_compute_fpfh.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_map_compute_spfh.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_cloud_compute_fpfh.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    lib.sf_features_match.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.sf_reg_default_params.restype = None
    lib.sf_cloud_register_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_cloud_pair_hypotheses.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_cloud_score_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_double, C.c_void_p]
    lib.sf_test_score_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_double, C.c_int, C.c_int64, C.c_void_p]
    lib.sf_iss_default_params.restype = None
    lib.sf_map_iss_saliency.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_map_iss_keypoints.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_cloud_iss_keypoints.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.sf_features_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.sf_ndt_default_params.restype = None
    lib.sf_ndt_default_params.argtypes = [C.c_void_p]
    lib.sf_ndt_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_ndt_destroy.argtypes = [C.c_void_p]
    lib.sf_ndt_destroy.restype = None
    lib.sf_ndt_set_target_cloud.argtypes = [C.c_void_p, C.c_void_p]
    lib.sf_ndt_set_target_map.argtypes = [C.c_void_p, C.c_void_p]
    lib.sf_ndt_download_voxels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.sf_ndt_set_source_cloud.argtypes = [C.c_void_p, C.c_void_p]
    lib.sf_ndt_set_source_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
    lib.sf_ndt_derivatives.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.sf_ndt_align.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_ndt_align_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_ndt_stats_read.argtypes = [C.c_void_p, C.c_void_p]
    lib.sf_ndt_default_line_search.restype = None
    lib.sf_ndt_default_line_search.argtypes = [C.c_void_p]
    lib.sf_ndt_set_line_search.argtypes = [C.c_void_p, C.c_void_p]
    lib.sf_ndt_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.sf_ndt_line_search_read.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.sf_ndt_align_levels.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_range_image_default_params.restype = None
    lib.sf_range_image_default_params.argtypes = [C.c_void_p]
    lib.sf_visibility_default_params.restype = None
    lib.sf_visibility_default_params.argtypes = [C.c_void_p]
    lib.sf_range_image_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_range_image_destroy.argtypes = [C.c_void_p]
    lib.sf_range_image_destroy.restype = None
    lib.sf_range_image_info.argtypes = [C.c_void_p, C.c_void_p]
    lib.sf_range_image_build.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_range_image_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_map_visibility.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_map_visibility_votes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_cloud_remove_seen_through.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.sf_place_default_params.restype = None
    lib.sf_place_default_params.argtypes = [C.c_void_p]
    lib.sf_cloud_scan_context.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_place_db_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_place_db_destroy.argtypes = [C.c_void_p]
    lib.sf_place_db_destroy.restype = None
    lib.sf_place_db_info.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_place_db_clear.argtypes = [C.c_void_p]
    lib.sf_place_db_add_cloud.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_place_db_add_descriptors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.sf_place_db_download.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.sf_place_db_distances.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_place_db_query.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_place_db_query_cloud.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_map_radius_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    lib.sf_map_radius_graph.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    lib.sf_map_radius_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.sf_map_set_radius_fill.argtypes = [C.c_void_p, C.c_int]
    lib.sf_map_radius_launch_ms.argtypes = [C.c_void_p, C.c_void_p]
    lib.sf_test_launch_schedule.argtypes =[C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    lib.sf_test_compact.argtypes = [C.c_void_p, C.c_void_p]
    lib.sf_test_cloud_minmax.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sf_test_query_order.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.sf_icp_test_download_cache.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _lib = lib
    return lib


def voxel_merge_min_points(n=-1):
    """Map size from which Cloud.voxel_merge merges instead of re-filtering (returns the previous value; n < 0 only reads it)."""
    return int(load_library().sf_cloud_voxel_merge_min_points(C.c_int64(n)))


def kernel_sources():
    """sf_icp.hip and every file of csrc/ it reaches through #include "..." lines (followed through the files found), sorted
    by name: what the translation unit of the dominant kernel is compiled from.  A quoted name that is no file of csrc/ is
    passed over (the public header lives in include/); tests/test_schedule_rule.py holds the result against the compiler's own list."""
    import re
    csrc = os.path.join(_HERE, "csrc")
    found, todo = set(), ["sf_icp.hip"]
    while todo:
        name = todo.pop()
        if name in found or not os.path.isfile(os.path.join(csrc, name)):
            continue
        found.add(name)
        with open(os.path.join(csrc, name), "r", encoding="utf-8", errors="replace") as f:
            todo += re.findall(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', f.read(), re.M)
    return sorted(found)


def kernel_source_hash():
    """sha256[:16] of the sources the dominant kernel (k_nn_red / k_ref_nn) is compiled from (kernel_sources).
    profiles/*_traffic.json carry the hash of the build their counters were taken on; bench.py only quotes them while it
    still matches."""
    import hashlib
    h = hashlib.sha256()
    for name in kernel_sources():
        with open(os.path.join(_HERE, "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def _check(rc):
    if rc != 0:
        raise SlamFusionError("libslamfusion error %d: %s" % (rc, load_library().sf_last_error().decode()))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


SCHEDULE_INPUTS = ("mode", "K", "qpl", "sharded", "whole", "reuse", "window", "robust", "wanted", "fz_from", "defer", "table", "nbr_from", "lk_min", "tile_on")
SCHEDULE_OUTPUTS = ("launches", "nn", "one_per_lane", "solve_takes_freeze_state", "ask_freeze", "deferred_rows", "attempt_from", "fz", "lookup_first", "defer_first")
NN_SEARCH, NN_TILE_SEARCH, NN_DEFERRING, NN_FREEZE, NN_FROZEN_FEW = range(5)


def hook_launch_schedule(configs, k):
    """Test hook (sf_test_launch_schedule): configs[rows][SCHEDULE_INPUTS] -> int32 [rows][SCHEDULE_OUTPUTS], the form of launch k
    under each configuration.  Host code alone: needs no device."""
    configs = np.ascontiguousarray(configs, dtype=np.int32).reshape(-1, len(SCHEDULE_INPUTS))
    out = np.empty((len(configs), len(SCHEDULE_OUTPUTS)), np.int32)
    _check(load_library().sf_test_launch_schedule(_p(configs), len(configs), int(k), _p(out)))
    return out


def hook_plane_score(cloud, planes, distance_threshold, max_blocks=0):
    """Test hook (sf_test_plane_score): Cloud.score_planes with the scoring grid capped at max_blocks workgroups (0: as in production)."""
    planes = _f32(planes).reshape(-1, 4)
    counts = np.empty(len(planes), np.int64)
    _check(cloud.lib.sf_test_plane_score(cloud.h, _p(planes), len(planes), float(distance_threshold), int(max_blocks), _p(counts)))
    return counts


def hook_score_poses(src, dst, pairs, T12, distance_threshold, max_blocks=0, pair_chunk=0):
    """Test hook (sf_test_score_poses): Cloud.score_poses with the first grid dimension of the scoring kernel capped at max_blocks
    workgroups and the pairs split into slices of pair_chunk (0: as in production)."""
    pairs, T12 = _pairs(pairs), _f32(T12).reshape(-1, 12)
    counts = np.empty(len(T12), np.int64)
    _check(src.lib.sf_test_score_poses(src.h, dst.h, _p(pairs), C.c_int64(len(pairs)), _p(T12), C.c_int64(len(T12)), C.c_double(distance_threshold), C.c_int(int(max_blocks)),
                                       C.c_int64(int(pair_chunk)), _p(counts)))
    return counts


def hook_label_boxes(cloud, labels, n_labels=None, mode="pca", up=None, max_blocks=0):
    """Test hook (sf_test_label_boxes): Cloud.label_boxes with the grid of the segmented passes capped at max_blocks workgroups (0: as
    in production) -> (boxes, stats dict)."""
    return cloud._label_boxes(labels, n_labels, mode, up, False, int(max_blocks))


def hook_radix_sort(ctx, keys, vals, end_bit, lead=0, lead_alt=0):
    """Test hook (sf_test_radix_sort): the library's stable radix sort on host arrays.  keys: uint32 or uint64; vals: uint32
    or None (keys only).  Returns (sorted keys, sorted vals or None, damaged guard words)."""
    keys = np.ascontiguousarray(keys)
    if keys.dtype not in (np.uint32, np.uint64):
        raise SlamFusionError("hook_radix_sort: keys must be uint32 or uint64, not %s" % keys.dtype)
    vals = None if vals is None else np.ascontiguousarray(vals, dtype=np.uint32)
    keys_out = np.empty_like(keys)
    vals_out = None if vals is None else np.empty_like(vals)
    damage = C.c_int64(-1)
    _check(ctx.lib.sf_test_radix_sort(ctx.h, keys.dtype.itemsize, _p(keys), None if vals is None else _p(vals), len(keys), int(end_bit), int(lead), int(lead_alt),
                                      _p(keys_out), None if vals is None else _p(vals_out), C.addressof(damage)))
    return keys_out, vals_out, damage.value


def hook_scan_u32(ctx, op, values, carry0=0, in_place=False):
    """Test hook (sf_test_scan_u32): the library's device scan of a uint32 array, op 0 = carry0 + exclusive sum, 1 = inclusive
    max with carry0.  Returns (scanned array, damaged guard words)."""
    values = np.ascontiguousarray(values, dtype=np.uint32)
    out = np.empty_like(values)
    damage = C.c_int64(-1)
    _check(ctx.lib.sf_test_scan_u32(ctx.h, int(op), _p(values), len(values), int(carry0), int(bool(in_place)), _p(out), C.addressof(damage)))
    return out, damage.value


# ops of sf_test_linalg: name -> (SF_TEST_OP_*, doubles read, doubles written per case)
LINALG_OPS = {"rsqrt": (0, 1, 2), "svd3": (1, 9, 21), "kabsch": (2, 32, 16), "ldlt6": (3, 42, 7), "vec6": (4, 6, 16),
              "jacobi3": (5, 9, 13), "jacobi6": (6, 36, 43), "robust": (7, 3, 1), "eigvec": (8, 9, 3)}


def hook_linalg(ctx, op, cases):
    """Test hook (sf_test_linalg): one production float64 routine per row of `cases` (rows of LINALG_OPS[op][1] doubles), one
    case per GPU thread.  Returns an array of LINALG_OPS[op][2] doubles per case."""
    code, n_in, n_out = LINALG_OPS[op]
    cases = _f64(cases).reshape(-1, n_in)
    out = np.zeros((len(cases), n_out))
    _check(ctx.lib.sf_test_linalg(ctx.h, code, _p(cases), n_in, len(cases), _p(out), n_out))
    return out


def hook_wave_reduce(ctx, width, values):
    """Test hook (sf_test_wave_reduce): values[256][width] -> what wave_reduce_<width> returned on each of the 256 lanes."""
    values = _f64(values).reshape(256, int(width))
    out = np.zeros(256)
    _check(ctx.lib.sf_test_wave_reduce(ctx.h, int(width), _p(values), _p(out)))
    return out


def hook_block_reduce(ctx, nrec, values, fill=0.0):
    """Test hook (sf_test_block_reduce): block_reduce_store<nrec> of values[256][nrec] into 32 doubles that start as `fill`."""
    values = _f64(values).reshape(256, int(nrec))
    out = np.full(32, fill, dtype=np.float64)
    _check(ctx.lib.sf_test_block_reduce(ctx.h, int(nrec), _p(values), _p(out)))
    return out


def hook_reduce_partials(ctx, nrec, nt, part):
    """Test hook (sf_test_reduce_partials): reduce_partials<nrec, nt> over part[nblocks][32] -> the 32 doubles of rec."""
    part = _f64(part).reshape(-1, 32)
    out = np.full(32, np.nan)
    _check(ctx.lib.sf_test_reduce_partials(ctx.h, int(nrec), int(nt), _p(part), len(part), _p(out)))
    return out


def hook_compact(cloud, flags):
    """Test hook (sf_test_compact): the stream compaction behind every crop and filter with flags of the caller's choosing (uint8, one
    per point, non-zero keeps), in place.  Returns (points, kept indices)."""
    flags = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
    if len(flags) != len(cloud):
        raise SlamFusionError("hook_compact: %d flags for %d points" % (len(flags), len(cloud)))
    _check(cloud.lib.sf_test_compact(cloud.h, _p(flags) if len(flags) else None))
    return cloud.download(), cloud.last_indices()


def hook_cloud_minmax(cloud, enqueue=False):
    """Test hook (sf_test_cloud_minmax): bounds of the finite points as the voxel grids take them (sf::cloud_minmax) or, enqueue=True,
    as the merge and the patch do (sf::cloud_minmax_enqueue).  Returns (mn float32[3], mx float32[3], finite points)."""
    mn, mx, cnt = np.full(3, np.nan, np.float32), np.full(3, np.nan, np.float32), C.c_int64(-1)
    _check(cloud.lib.sf_test_cloud_minmax(cloud.h, int(bool(enqueue)), _p(mn), _p(mx), C.addressof(cnt)))
    return mn, mx, cnt.value


def hook_query_order(map_, points, poses=None, form=1, table=False):
    """Test hook (sf_test_query_order): the query ordering of an alignment on host scans points[B][n][3] under one 4x4 pose per scan
    (default: identity), form 0 = k_order_scatter + k_order_gather, 1 = k_order_move; table: the density-equalised buckets of the
    map's index instead of the plain cell key.  Returns (keys uint16 [B][n] in element order, ordered float32 [B][n][3])."""
    points = _f32(points)
    if points.ndim != 3 or points.shape[2] != 3:
        raise SlamFusionError("hook_query_order: points must be [B][n][3], not %r" % (points.shape,))
    batch, n = points.shape[:2]
    poses = np.tile(np.eye(4), (batch, 1, 1)) if poses is None else _f64(poses).reshape(batch, 4, 4)
    poses = _f64(poses)
    keys = np.empty((batch, n), np.uint16)
    ordered = np.empty((batch, n, 3), np.float32)
    _check(map_.lib.sf_test_query_order(map_.h, _p(points), batch, n, _p(poses), int(form), int(bool(table)), _p(keys), _p(ordered)))
    return keys, ordered


def _pc2_layout(msg):
    """(buffer, width, height, point_step, row_step, (off_x, off_y, off_z), datatype, is_bigendian) of a PointCloud2-like message"""
    offs, types = {"x": 0, "y": 4, "z": 8}, {"x": 7, "y": 7, "z": 7}
    for f in getattr(msg, "fields", []) or []:
        if f.name in offs:
            offs[f.name] = int(f.offset)
            types[f.name] = int(getattr(f, "datatype", 7))
    if len(set(types.values())) != 1:
        raise SlamFusionError("PointCloud2 x/y/z fields have different datatypes: %r" % (types,))
    buf = np.frombuffer(msg.data, dtype=np.uint8)
    return (buf, int(msg.width), int(msg.height), int(msg.point_step), int(getattr(msg, "row_step", 0) or 0), (offs["x"], offs["y"], offs["z"]), types["x"],
            int(bool(getattr(msg, "is_bigendian", False))))


class Context:
    """sf_ctx: one device + one HIP stream (optionally a caller-owned stream)."""

    def __init__(self, device=0, stream=None):
        self.lib = load_library()
        self.h = C.c_void_p()
        _check(self.lib.sf_ctx_create(C.c_int(device), C.c_void_p(stream), C.byref(self.h)))
        _live.add(self)

    def synchronize(self):
        _check(self.lib.sf_ctx_synchronize(self.h))

    @property
    def stream(self):
        return self.lib.sf_ctx_stream(self.h)

    def device_name(self):
        buf = C.create_string_buffer(256)
        _check(self.lib.sf_ctx_device_name(self.h, buf, C.c_int(256)))
        return buf.value.decode()

    def close(self):
        if self.h:
            self.lib.sf_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Cloud:
    """sf_cloud: device point set with the reference's preprocessing operations."""

    def __init__(self, ctx, xyz=None):
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p()
        _check(self.lib.sf_cloud_create(ctx.h, C.byref(self.h)))
        _live.add(self)
        if xyz is not None:
            self.upload(xyz)

    def upload(self, xyz):
        xyz = _f32(xyz).reshape(-1, 3)
        _check(self.lib.sf_cloud_upload(self.h, _p(xyz), C.c_int64(len(xyz))))
        return self

    def upload_async_ptr(self, host_ptr, n):
        """n x 3 float32 at a raw host address, enqueue only (pinned memory: asynchronous, stream-ordered)"""
        _check(self.lib.sf_cloud_upload_async(self.h, C.c_void_p(host_ptr), C.c_int64(n)))
        return self

    def device_ptr(self):
        return self.lib.sf_cloud_device_ptr(self.h)

    def from_pointcloud2(self, msg):
        """PointCloud2-like message (width, height, point_step, row_step, is_bigendian, fields or x/y/z float32 at
        0/4/8, data).  The buffer length, the x/y/z datatype (FLOAT32 = 7 or FLOAT64 = 8, all three alike) and the
        endianness are checked here and again behind the C ABI."""
        buf, width, height, point_step, row_step, offs, dtype, big = _pc2_layout(msg)
        _check(self.lib.sf_cloud_from_pointcloud2_msg(self.h, _p(buf), C.c_int64(buf.size), C.c_int64(width), C.c_int64(height), C.c_int(point_step), C.c_int64(row_step),
                                                      C.c_int(offs[0]), C.c_int(offs[1]), C.c_int(offs[2]), C.c_int(dtype), C.c_int(big)))
        return self

    def load_pcd(self, path):
        _check(self.lib.sf_cloud_load_pcd(self.h, str(path).encode()))
        return self

    def save_pcd(self, path):
        _check(self.lib.sf_cloud_save_pcd(self.h, str(path).encode()))

    def from_device(self, ptr, n):
        _check(self.lib.sf_cloud_from_device(self.h, C.c_void_p(ptr), C.c_int64(n)))
        return self

    def __len__(self):
        n = C.c_int64()
        _check(self.lib.sf_cloud_size(self.h, C.byref(n)))
        return n.value

    def download(self):
        n = len(self)
        out = np.empty((n, 3), np.float32)
        _check(self.lib.sf_cloud_download(self.h, _p(out), C.c_int64(n), None))
        return out

    def copy(self):
        c = Cloud(self.ctx)
        _check(self.lib.sf_cloud_copy(c.h, self.h))
        return c

    def copy_from(self, other):
        """device-to-device copy into this cloud's own (persistent) buffer"""
        _check(self.lib.sf_cloud_copy(self.h, other.h))
        return self

    def subsample(self, step):                       # applyUniformSubsample
        _check(self.lib.sf_cloud_subsample(self.h, C.c_int(step)))
        return self

    def crop_radius(self, center, radius, sorted=False):  # cropPointCloudThroughRadius
        c = _f32(center)
        _check(self.lib.sf_cloud_crop_radius(self.h, _p(c), C.c_double(radius), C.c_int(int(sorted))))
        return self

    def remove_floor(self):                          # removeFloor
        _check(self.lib.sf_cloud_remove_floor(self.h))
        return self

    def crop_aabb(self, lo, hi):                     # readFilterPtcRegionPoints
        lo, hi = _f64(lo), _f64(hi)
        _check(self.lib.sf_cloud_crop_aabb(self.h, _p(lo), _p(hi)))
        return self

    def crop_obb(self, center, R, extent):           # OrientedBoundingBox crop
        c, R, e = _f64(center), _f64(R).reshape(3, 3), _f64(extent)
        _check(self.lib.sf_cloud_crop_obb(self.h, _p(c), _p(R), _p(e)))
        return self

    def append(self, other):                         # *map_cloud += *cloud
        _check(self.lib.sf_cloud_append(self.h, other.h))
        return self

    def transform(self, T):                          # applyTransformation
        T = _f32(T).reshape(16)
        _check(self.lib.sf_cloud_transform(self.h, _p(T)))
        return self

    def remove_statistical_outliers(self, nb_neighbors=20, std_ratio=2.0, flavour="pcl", cell=0.0):
        """sf_cloud_remove_statistical_outliers (pcl::StatisticalOutlierRemoval / Open3D remove_statistical_outlier): in place, order
        kept, `last_indices` reports the survivors -> stats dict.  `cell`: the cell of the temporary index (0 = automatic)."""
        st = OutlierStats()
        _check(self.lib.sf_cloud_remove_statistical_outliers(self.h, C.c_int(int(nb_neighbors)), C.c_double(std_ratio), C.c_int(_sor_flavour(flavour)), C.c_float(cell),
                                                             C.byref(st)))
        return st.as_dict()

    def remove_radius_outliers(self, radius, min_neighbors, cell=0.0):
        """sf_cloud_remove_radius_outliers (pcl::RadiusOutlierRemoval / Open3D remove_radius_outlier): keeps the points with more than
        `min_neighbors` other points within `radius` -> stats dict."""
        st = OutlierStats()
        _check(self.lib.sf_cloud_remove_radius_outliers(self.h, C.c_double(radius), C.c_int(int(min_neighbors)), C.c_float(cell), C.byref(st)))
        return st.as_dict()

    def filter_clusters(self, tolerance, min_size, max_size=0, cell=0.0):
        """sf_cloud_filter_clusters (pcl::EuclideanClusterExtraction as a filter): keeps the points whose connected piece at `tolerance`
        has min_size .. max_size points (max_size <= 0: no upper bound); in place, order kept, `last_indices` reports the survivors
        -> stats dict.  `cell`: the cell of the temporary index (0 = automatic)."""
        st = ClusterStats()
        _check(self.lib.sf_cloud_filter_clusters(self.h, C.c_double(tolerance), C.c_int64(int(min_size)), C.c_int64(int(max_size)), C.c_float(cell), C.byref(st)))
        return st.as_dict()

    def keep_largest_cluster(self, tolerance, cell=0.0):
        """sf_cloud_keep_largest_cluster: keeps the connected piece with the most points (a tie: the one holding the earliest point)
        -> stats dict with n_kept = largest_size."""
        st = ClusterStats()
        _check(self.lib.sf_cloud_keep_largest_cluster(self.h, C.c_double(tolerance), C.c_float(cell), C.byref(st)))
        return st.as_dict()

    def plane_hypotheses(self, num_hypotheses=1024, seed=0, axis=None, max_angle_deg=None):
        """sf_cloud_plane_hypotheses: the planes a segmentation with these parameters scores -> (planes float32 [H, 4], a degenerate
        one four NaNs; samples int32 [H, 3], the original indices; the number of degenerate hypotheses)."""
        p = _plane_params(0.1, num_hypotheses, True, seed, 3, axis, max_angle_deg, False)
        h = max(int(num_hypotheses), 0)
        planes, samples, n_deg = np.empty((h, 4), np.float32), np.empty((h, 3), np.int32), C.c_int64()
        _check(self.lib.sf_cloud_plane_hypotheses(self.h, C.byref(p), _p(planes), _p(samples), C.byref(n_deg)))
        return planes, samples, n_deg.value

    def score_planes(self, planes, distance_threshold):
        """sf_cloud_score_planes: the inliers of each plane (a, b, c, d) under the score rule -> int64 [len(planes)]."""
        planes = _f32(planes).reshape(-1, 4)
        counts = np.empty(len(planes), np.int64)
        _check(self.lib.sf_cloud_score_planes(self.h, _p(planes), C.c_int64(len(planes)), C.c_double(distance_threshold), _p(counts)))
        return counts

    def segment_plane(self, distance_threshold=0.1, num_hypotheses=1024, refine=True, seed=0, min_inliers=3, axis=None, max_angle_deg=None, profile=False):
        """sf_cloud_segment_plane (pcl::SACSegmentation with SACMODEL_PLANE, or SACMODEL_PERPENDICULAR_PLANE with `axis` and
        `max_angle_deg`; Open3D segment_plane): the plane with the most points within `distance_threshold` among `num_hypotheses`
        three-point samples, refitted to its inliers -> (plane float32 [4], inlier mask bool [n], stats dict).  The cloud stays as it
        is.  No plane with min_inliers points: stats["found"] = 0, the plane is zeros, no inlier."""
        p = _plane_params(distance_threshold, num_hypotheses, refine, seed, min_inliers, axis, max_angle_deg, profile)
        plane, inlier, st = np.zeros(4, np.float32), np.zeros(len(self), np.uint8), PlaneStats()
        _check(self.lib.sf_cloud_segment_plane(self.h, C.byref(p), _p(plane), _p(inlier), C.byref(st)))
        return plane, inlier.astype(bool), st.as_dict()

    def remove_plane(self, distance_threshold=0.1, num_hypotheses=1024, refine=True, seed=0, min_inliers=3, axis=None, max_angle_deg=None, profile=False,
                     keep_inliers=False):
        """sf_cloud_remove_plane: segment_plane, then the inliers are taken out (keep_inliers: everything else is) in place, order
        kept, `last_indices` reports the survivors -> (plane, stats dict).  Nothing is removed when no plane is found."""
        p = _plane_params(distance_threshold, num_hypotheses, refine, seed, min_inliers, axis, max_angle_deg, profile)
        plane, st = np.zeros(4, np.float32), PlaneStats()
        _check(self.lib.sf_cloud_remove_plane(self.h, C.byref(p), C.c_int(int(bool(keep_inliers))), _p(plane), C.byref(st)))
        return plane, st.as_dict()

    def _label_boxes(self, labels, n_labels, mode, up, profile, max_blocks):
        labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        if len(labels) != len(self):
            raise SlamFusionError("labels must have one entry per point (%d, got %d)" % (len(self), len(labels)))
        if n_labels is None:
            n_labels = int(labels.max()) + 1 if len(labels) and labels.max() >= 0 else 0
        p, st = _box_params(mode, up, profile), BoxStats()
        boxes = np.zeros(max(int(n_labels), 0), LABEL_BOX_DTYPE)
        if max_blocks is None:
            rc = self.lib.sf_cloud_label_boxes(self.h, _p(labels), C.c_int64(int(n_labels)), C.byref(p), _p(boxes), C.byref(st))
        else:
            rc = self.lib.sf_test_label_boxes(self.h, _p(labels), C.c_int64(int(n_labels)), C.byref(p), C.c_int(max_blocks), _p(boxes), C.byref(st))
        _check(rc)
        return boxes, st.as_dict()

    def label_boxes(self, labels, n_labels=None, mode="pca", up=None, profile=False):
        """sf_cloud_label_boxes (PCL getMinMax3D / MomentOfInertiaEstimation, Open3D get_axis_aligned_bounding_box /
        get_oriented_bounding_box, per label): labels int32 [n], a member is a finite point with 0 <= label < n_labels (None: the largest
        label + 1) -> (structured array [n_labels] of LABEL_BOX_DTYPE: count, lo, hi, mean, cov, center, R, extent, eigenvalues, valid;
        stats dict).  mode "aabb" | "pca" | "upright" (axes about `up`, None = +z).  The cloud stays as it is."""
        return self._label_boxes(labels, n_labels, mode, up, profile, None)

    def cluster_boxes(self, tolerance, min_size=1, max_size=0, cell=0.0, mode="pca", up=None):
        """sf_cloud_cluster_boxes: the boxes of the Euclidean clusters at `tolerance` (Map.cluster_euclidean's labels, which never leave
        the device) -> (structured array [n_clusters] in label order, cluster stats dict, box stats dict).  The cloud stays as it is."""
        p, cst, bst = _box_params(mode, up, False), ClusterStats(), BoxStats()
        args = (self.h, C.c_double(tolerance), C.c_int64(int(min_size)), C.c_int64(int(max_size)), C.c_float(cell), C.byref(p))
        boxes = np.zeros(min(len(self), 4096), LABEL_BOX_DTYPE)
        _check(self.lib.sf_cloud_cluster_boxes(*args, _p(boxes), C.c_int64(len(boxes)), C.byref(cst), C.byref(bst)))
        if cst.n_clusters > len(boxes):                     # more clusters than the first buffer holds: once more with room for all
            boxes = np.zeros(int(cst.n_clusters), LABEL_BOX_DTYPE)
            _check(self.lib.sf_cloud_cluster_boxes(*args, _p(boxes), C.c_int64(len(boxes)), C.byref(cst), C.byref(bst)))
        return boxes[:int(cst.n_clusters)].copy(), cst.as_dict(), bst.as_dict()

    def remove_boxes(self, boxes_or_arrays, margin=0.0, keep_inside=False):
        """sf_cloud_remove_boxes: takes out the points inside at least one box (keep_inside: everything else), each box grown by
        `margin` on every side; in place, order kept, `last_indices` reports the survivors -> the number of points inside.
        boxes_or_arrays: a structured array of label_boxes / cluster_boxes (its valid entries are used) or (center [B, 3], R [B, 3, 3],
        extent [B, 3]); at most 1024 boxes."""
        if isinstance(boxes_or_arrays, np.ndarray) and boxes_or_arrays.dtype.names:
            b = boxes_or_arrays[boxes_or_arrays["valid"] != 0]
            center, R, extent = b["center"], b["R"], b["extent"]
        else:
            center, R, extent = boxes_or_arrays
        center, R, extent = _f64(center).reshape(-1, 3), _f64(R).reshape(-1, 9), _f64(extent).reshape(-1, 3)
        if not len(center) == len(R) == len(extent):
            raise SlamFusionError("center, R and extent must describe the same number of boxes")
        n_inside = C.c_int64()
        _check(self.lib.sf_cloud_remove_boxes(self.h, _p(center), _p(R), _p(extent), C.c_int64(len(center)), C.c_double(margin), C.c_int(int(bool(keep_inside))),
                                              C.byref(n_inside)))
        return n_inside.value

    def remove_seen_through(self, images, poses, min_seen=1, max_within=0, half_cols=1, half_rows=1, min_hits=1, range_margin=0.2, range_ratio=0.01, profile=False):
        """sf_cloud_remove_seen_through: takes out the points that at least min_seen of the range images (RangeImage objects, with
        poses [B, 4, 4] map <- sensor of the scans they were built from) class SEEN_THROUGH and at most max_within class WITHIN; in
        place, order kept, `last_indices` reports the survivors -> stats dict (n_removed: the points taken away).  A cleaned map is
        this call on the map's cloud, then Map.build."""
        handles, poses, b = _images_and_poses(images, poses)
        p, st = _visibility_params(half_cols, half_rows, min_hits, range_margin, range_ratio, profile), VisibilityStats()
        _check(self.lib.sf_cloud_remove_seen_through(self.h, handles, _p(poses) if poses is not None else None, C.c_int64(b), C.byref(p), C.c_int(int(min_seen)),
                                                     C.c_int(int(max_within)), C.byref(st)))
        return st.as_dict()

    def scan_context(self, pose=None, **params):
        """sf_cloud_scan_context: the Scan Context descriptor of the cloud seen from `pose` ([4, 4] parent <- sensor; None: the cloud
        is in the sensor frame already); params: num_rings, num_sectors, min_range, max_range, sensor_height ->
        (float32 [num_rings, num_sectors] of maximum heights, +0 where empty; stats dict)."""
        p, st = _scan_context_params(**params), ScanContextStats()
        desc = np.zeros((max(p.num_rings, 0), max(p.num_sectors, 0)), np.float32)
        pose = None if pose is None else _f64(pose).reshape(16)
        _check(self.lib.sf_cloud_scan_context(self.h, _p(pose) if pose is not None else None, C.byref(p), _p(desc), C.byref(st)))
        return desc, st.as_dict()

    def compute_fpfh(self, normal_radius, radius, orient="none", toward=(0, 0, 1), cell=0.0, profile=False):
        """sf_cloud_compute_fpfh: a temporary map of the cloud, Map.estimate_normals(normal_radius) on it, then Map.compute_fpfh(radius,
        orient, toward) -> (Features in the cloud's point order, stats dict); bit for bit what those three calls give.  The cloud stays
        as it is."""
        p, st, out = _fpfh_params(radius, orient, toward, profile), FpfhStats(), Features(self.ctx)
        _check(self.lib.sf_cloud_compute_fpfh(self.h, C.c_double(normal_radius), C.byref(p), C.c_float(cell), out.h, C.byref(st)))
        return out, st.as_dict()

    def iss_keypoints(self, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, min_lambda3=0.0, profile=False, cell=0.0):
        """sf_cloud_iss_keypoints: a temporary map of the cloud, then Map.iss_keypoints -> dict(indices int32 [k] ascending, stats);
        bit for bit what those two calls give.  The cloud and its last indices stay as they are."""
        p, st, n, nk = _iss_params(salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors, min_lambda3, profile), IssStats(), len(self), C.c_int64()
        idx = np.zeros(max(n, 1), np.int32)
        _check(self.lib.sf_cloud_iss_keypoints(self.h, C.byref(p), C.c_float(cell), _p(idx), C.c_int64(n), C.byref(nk), C.byref(st)))
        return dict(indices=idx[:nk.value].copy(), stats=st.as_dict())

    def pair_hypotheses(self, other, pairs, edge_similarity=0.9, num_hypotheses=4096, seed=0):
        """sf_cloud_pair_hypotheses: the hypotheses a register_pairs with these parameters builds -> (samples int32 [H, 3], the sampled
        pairs; status int32 [H]: 0, 1 degenerate, 2 rejected by the edge check; T float64 [H, 4, 4], NaN unless status 0)."""
        pairs, p = _pairs(pairs), _reg_params(1.0, edge_similarity, num_hypotheses, 0, 3, 0, seed, False)
        h = max(int(num_hypotheses), 0)
        samples, status, T = np.empty((h, 3), np.int32), np.empty(h, np.int32), np.empty((h, 4, 4), np.float64)
        _check(self.lib.sf_cloud_pair_hypotheses(self.h, other.h, _p(pairs), C.c_int64(len(pairs)), C.byref(p), _p(samples), _p(status), _p(T)))
        return samples, status, T

    def score_poses(self, other, pairs, T12, distance_threshold):
        """sf_cloud_score_poses: the pairs each float32 transform (the rows of [R | t], [H, 12] or [H, 3, 4]) brings within
        distance_threshold under the score rule -> int64 [H]."""
        pairs, T12 = _pairs(pairs), _f32(T12).reshape(-1, 12)
        counts = np.empty(len(T12), np.int64)
        _check(self.lib.sf_cloud_score_poses(self.h, other.h, _p(pairs), C.c_int64(len(pairs)), _p(T12), C.c_int64(len(T12)), C.c_double(distance_threshold), _p(counts)))
        return counts

    def register_pairs(self, other, pairs, distance_threshold, edge_similarity=0.9, num_hypotheses=4096, refine_rounds=2, min_inliers=3, top_k=0, seed=0,
                       profile=False):
        """sf_cloud_register_pairs (pcl::SampleConsensusPrerejective, Open3D registration_ransac_based_on_correspondence): the pose
        that maps this cloud into `other`, estimated from the matched pairs (i into this cloud, j into other, as Features.match returns
        them): three-pair hypotheses, the edge-length pre-rejection, inlier counts over all pairs, a least-squares refit over the
        inliers -> dict(T float64 [4, 4], found, inlier bool [m], top: list of dict(h, status, count, T), stats).  Neither cloud is
        modified.  No hypothesis with min_inliers: found = 0, T the identity, no inlier."""
        pairs, p = _pairs(pairs), _reg_params(distance_threshold, edge_similarity, num_hypotheses, refine_rounds, min_inliers, top_k, seed, profile)
        T, inlier, st = np.zeros((4, 4), np.float64), np.zeros(len(pairs), np.uint8), RegStats()
        top = (RegCandidate * max(int(top_k), 1))()
        _check(self.lib.sf_cloud_register_pairs(self.h, other.h, _p(pairs), C.c_int64(len(pairs)), C.byref(p), _p(T), _p(inlier), top, C.byref(st)))
        return dict(T=T, found=int(st.found), inlier=inlier.astype(bool), top=[top[k].as_dict() for k in range(int(st.n_top))], stats=st.as_dict())

    def last_indices(self):
        n = C.c_int64()
        cap = 1 << 20
        while True:
            out = np.empty(cap, np.int32)
            rc = self.lib.sf_cloud_last_indices(self.h, _p(out), C.c_int64(cap), C.byref(n))
            if rc == 0:
                return out[:n.value].copy()
            if n.value > cap:
                cap = n.value
                continue
            _check(rc)

    def voxel_downsample(self, leaf=0.1, flavour="pcl"):
        flags = C.c_int(0)
        fl = {"pcl": SF_VOXEL_PCL, "o3d": SF_VOXEL_O3D, "pcl64": SF_VOXEL_PCL64}[flavour]
        _check(self.lib.sf_cloud_voxel_downsample(self.h, C.c_double(leaf), C.c_int(fl), C.byref(flags)))
        return flags.value

    def voxel_merge(self, pending, leaf=0.1):
        """append(pending) + voxel_downsample(leaf, "pcl") as a merge when this cloud is already voxel-filtered -> (status flags, merged?)"""
        st, mg = C.c_int(), C.c_int()
        _check(self.lib.sf_cloud_voxel_merge(self.h, pending.h, C.c_double(leaf), C.byref(st), C.byref(mg)))
        return st.value, bool(mg.value)

    def _i32(self, fn):
        n = C.c_int64()
        fn(self.h, None, C.c_int64(0), C.byref(n))
        out = np.empty(max(n.value, 1), np.int32)
        _check(fn(self.h, _p(out), C.c_int64(len(out)), C.byref(n)))
        return out[:n.value]

    def _i64(self, fn):
        n = C.c_int64()
        fn(self.h, None, C.c_int64(0), C.byref(n))
        out = np.empty(max(n.value, 1), np.int64)
        _check(fn(self.h, _p(out), C.c_int64(len(out)), C.byref(n)))
        return out[:n.value]

    def voxel_point_ids64(self):                     # after voxel_downsample(flavour="pcl64")
        return self._i64(self.lib.sf_cloud_voxel_point_ids64)

    def voxel_out_ids64(self):
        return self._i64(self.lib.sf_cloud_voxel_out_ids64)

    def voxel_point_ids(self):
        return self._i32(self.lib.sf_cloud_voxel_point_ids)

    def voxel_out_ids(self):
        return self._i32(self.lib.sf_cloud_voxel_out_ids)

    def voxel_out_means_f64(self):
        n = C.c_int64()
        self.lib.sf_cloud_voxel_out_means_f64(self.h, None, C.c_int64(0), C.byref(n))
        out = np.empty((max(n.value, 1), 3), np.float64)
        _check(self.lib.sf_cloud_voxel_out_means_f64(self.h, _p(out), C.c_int64(len(out)), C.byref(n)))
        return out[:n.value]

    def close(self):
        if self.h:
            self.lib.sf_cloud_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Map:
    """sf_map: whole-map uniform-grid NN index (replaces the per-crop FLANN kd-tree)."""

    def __init__(self, ctx, cloud=None, cell=0.0):
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p()
        _check(self.lib.sf_map_create(ctx.h, C.byref(self.h)))
        _live.add(self)
        if cloud is not None:
            self.build(cloud, cell)

    def build(self, cloud, cell=0.0):
        if not isinstance(cloud, Cloud):
            cloud = Cloud(self.ctx, cloud)
        _check(self.lib.sf_map_build(self.h, cloud.h, C.c_float(cell)))
        return self

    def set_origin_lattice(self, cells):
        """sf_map_set_origin_lattice: the grid origin snapped down to a multiple of `cells` cells (0 = off), from the next build on."""
        _check(self.lib.sf_map_set_origin_lattice(self.h, C.c_int(int(cells))))
        return self

    def patch(self, cloud):
        """sf_map_patch: the index after the last `cloud.voxel_merge(...)`, merged from the old one when it can be; -> True if it was."""
        done = C.c_int(0)
        _check(self.lib.sf_map_patch(self.h, cloud.h, C.byref(done)))
        self.last_patch = done.value                          # 1 merged, SF_PATCH_* (<= 0): built, and why (include/slamfusion.h)
        return done.value > 0

    def index(self):
        """The index as it lies on the device (parity tests): dict(pts4 [n, 4] float32 with the point id bit-cast into column 3,
        cell_start [cells + 1] uint32, org, inv_h, gap_eps)."""
        n, nc, org, inv_h, eps = C.c_int64(), C.c_int64(), (C.c_float * 3)(), C.c_float(), C.c_float()
        _check(self.lib.sf_map_index_info(self.h, C.byref(n), C.byref(nc), org, C.byref(inv_h), C.byref(eps)))
        pts4 = np.empty((max(n.value, 1), 4), np.float32)
        cs = np.empty(nc.value + 1, np.uint32)
        _check(self.lib.sf_map_download_index(self.h, pts4.ctypes.data_as(C.c_void_p), C.c_int64(len(pts4)), cs.ctypes.data_as(C.c_void_p), C.c_int64(len(cs))))
        return dict(pts4=pts4[:n.value], cell_start=cs, org=np.array(list(org), np.float32), inv_h=inv_h.value, gap_eps=eps.value)

    def __len__(self):
        n = C.c_int64()
        _check(self.lib.sf_map_size(self.h, C.byref(n)))
        return n.value

    def cell_size(self):
        cell = C.c_float()
        dims = (C.c_int32 * 3)()
        _check(self.lib.sf_map_cell_size(self.h, C.byref(cell), dims))
        return cell.value, tuple(dims)

    def window_none(self):
        _check(self.lib.sf_map_window_none(self.h))

    def window_sphere(self, center, radius):
        c = _f32(center)
        _check(self.lib.sf_map_window_sphere(self.h, _p(c), C.c_double(radius)))

    def window_obb(self, center, R, extent):
        c, R, e = _f64(center), _f64(R).reshape(3, 3), _f64(extent)
        _check(self.lib.sf_map_window_obb(self.h, _p(c), _p(R), _p(e)))

    def window_count(self):
        n = C.c_int64()
        _check(self.lib.sf_map_window_count(self.h, C.byref(n)))
        return n.value

    def estimate_normals(self, radius, covariance=False):
        _check(self.lib.sf_map_estimate_normals_cov(self.h, C.c_float(radius), C.c_int(int(covariance))))

    def estimate_normals_knn(self, k, max_radius=np.inf, covariance=False):
        """sf_map_estimate_normals_knn: PCA normals (and covariances) from each map point's k nearest map points, itself included,
        within max_radius (inf or <= 0: no limit) -- Open3D's KDTreeSearchParamKNN / Hybrid."""
        r = float(max_radius)
        _check(self.lib.sf_map_estimate_normals_knn(self.h, C.c_int(int(k)), C.c_float(r if np.isfinite(r) else 0.0), C.c_int(int(covariance))))

    def set_normals_carry(self, on=True):
        """sf_map_set_normals_carry: `patch` keeps the estimated normals (and covariances) -- carried with the entries that stay,
        re-estimated where the merge changed a neighbourhood; bit-equal to patch + estimate_normals with the last arguments."""
        _check(self.lib.sf_map_set_normals_carry(self.h, C.c_int(int(bool(on)))))
        return self

    def normals_carry_info(self):
        """sf_map_normals_carry_info of the last `patch`: (how, changed positions, points re-estimated, map points); how = 1 carried,
        0 re-estimated in full (the patch took the build), -1 dropped."""
        out = (C.c_int64 * 4)()
        _check(self.lib.sf_map_normals_carry_info(self.h, out))
        return tuple(int(v) for v in out)

    def download_covariances(self):
        """[n, 6] float64: xx xy xz yy yz zz of each point's neighbourhood (original point order)."""
        n = len(self)
        cov = np.empty((n, 6), np.float64)
        _check(self.lib.sf_map_download_covariances(self.h, _p(cov), C.c_int64(n), None))
        return cov

    def set_normals(self, normals):
        nrm = _f32(normals).reshape(-1, 3)
        _check(self.lib.sf_map_set_normals(self.h, _p(nrm), C.c_int64(len(nrm))))

    def download_normals(self):
        n = len(self)
        nrm = np.empty((n, 3), np.float32)
        cnt = np.empty(n, np.int32)
        _check(self.lib.sf_map_download_normals(self.h, _p(nrm), _p(cnt), C.c_int64(n), None))
        return nrm, cnt

    def nn(self, queries, max_d2=np.inf):
        q = _f32(queries).reshape(-1, 3)
        idx = np.empty(len(q), np.int32)
        d2 = np.empty(len(q), np.float32)
        _check(self.lib.sf_map_nn(self.h, _p(q), C.c_int64(len(q)), C.c_float(min(max_d2, 3.0e38)), _p(idx), _p(d2)))
        return idx, d2

    def knn(self, queries, k, max_d2=np.inf):
        """sf_map_knn: the exact k nearest indexed points of each query (inside the window, d2 < max_d2) -> (idx [n, k] int32 in
        original point order, d2 [n, k] float32, count [n] int32); rows ascend in (d2, index position), tails are -1 / inf."""
        q = _f32(queries).reshape(-1, 3)
        k = int(k)
        rows = max(k, 0)
        idx = np.empty((len(q), rows), np.int32)
        d2 = np.empty((len(q), rows), np.float32)
        cnt = np.empty(len(q), np.int32)
        _check(self.lib.sf_map_knn(self.h, _p(q), C.c_int64(len(q)), C.c_int(k), C.c_float(max_d2), _p(idx), _p(d2), _p(cnt)))
        return idx, d2, cnt

    def _radius_rows(self, rows, call):
        offsets = np.zeros(rows + 1, np.int64)
        st, total = RadiusStats(), C.c_int64()
        _check(call(_p(offsets), C.byref(st)))
        idx = np.empty(int(st.total), np.int32)
        d2 = np.empty(int(st.total), np.float32)
        _check(self.lib.sf_map_radius_results(self.h, _p(idx), _p(d2), C.c_int64(len(idx)), C.byref(total)))
        assert total.value == len(idx) == offsets[-1]
        return offsets, idx, d2, st.as_dict()

    def radius_search(self, queries, radius, order="index"):
        """sf_map_radius_search (pcl radiusSearch, Open3D search_radius_vector_3d): every indexed point the window accepts with float32
        d2 < float32(radius^2) of each query -> (offsets int64 [n + 1], idx int32 [total] in original point order, d2 float32 [total],
        stats dict); row i is idx[offsets[i]:offsets[i + 1]].  order "index": rows ascend in position in the index; "distance": in
        (d2, position), the order of knn, so a row's first 64 entries are knn(q, 64, float32(radius^2))."""
        q = _f32(queries).reshape(-1, 3)
        o = _radius_order(order)
        return self._radius_rows(len(q), lambda off, st: self.lib.sf_map_radius_search(self.h, _p(q), C.c_int64(len(q)), C.c_double(radius), C.c_int(o), off, st))

    def radius_graph(self, radius, order="index"):
        """sf_map_radius_graph: radius_search of the map's own points without the window, row i for original point i (itself
        included; empty for a point that is not indexed); the row lengths are radius_outliers' n_neighbors."""
        o = _radius_order(order)
        return self._radius_rows(len(self), lambda off, st: self.lib.sf_map_radius_graph(self.h, C.c_double(radius), C.c_int(o), off, st))

    def hybrid_search(self, queries, radius, max_nn):
        """Open3D search_hybrid_vector_3d: at most max_nn nearest indexed points within radius = knn(queries, max_nn,
        float32(radius^2)) -> (idx [n, max_nn], d2 [n, max_nn], count [n])."""
        if not 1 <= int(max_nn) <= SF_KNN_MAX:
            raise ValueError("hybrid_search: max_nn must be 1 .. %d (got %r)" % (SF_KNN_MAX, max_nn))
        return self.knn(queries, int(max_nn), np.float32(float(radius) * float(radius)))

    def set_radius_fill(self, mode="auto"):
        """sf_map_set_radius_fill: "auto" (default: the form measured faster), "lane" (one lane per row) or "wave" (one wave per row);
        the rows are the same bytes either way."""
        _check(self.lib.sf_map_set_radius_fill(self.h, C.c_int(RADIUS_FILLS[mode] if mode in RADIUS_FILLS else int(mode))))
        return self

    def radius_launch_ms(self):
        """sf_map_radius_launch_ms: (count + scan, fill, sort) device ms of the last radius call; zeros unless profile_launches is on."""
        ms = (C.c_float * 3)()
        _check(self.lib.sf_map_radius_launch_ms(self.h, ms))
        return tuple(float(v) for v in ms)

    def statistical_outliers(self, k, std_ratio=2.0, flavour="pcl"):
        """sf_map_statistical_outliers: -> (keep bool [n], mean_dist float64 [n], stats dict), original point order.  flavour "pcl":
        k other points, keep iff d <= mean + std_ratio * stddev (pcl::StatisticalOutlierRemoval); "o3d": k points with the point
        itself among them, keep iff d < threshold (remove_statistical_outlier).  Points that are not indexed: False / NaN."""
        n = len(self)
        keep = np.zeros(n, np.uint8)
        dist = np.empty(n, np.float64)
        st = OutlierStats()
        _check(self.lib.sf_map_statistical_outliers(self.h, C.c_int(int(k)), C.c_double(std_ratio), C.c_int(_sor_flavour(flavour)), _p(keep), _p(dist), C.byref(st)))
        return keep.astype(bool), dist, st.as_dict()

    def radius_outliers(self, radius, min_neighbors):
        """sf_map_radius_outliers: -> (keep bool [n], n_neighbors int32 [n], stats dict), original point order.  n_neighbors counts the
        indexed points with float32 d2 < float32(radius^2), the point itself included; keep iff n_neighbors > min_neighbors."""
        n = len(self)
        keep = np.zeros(n, np.uint8)
        cnt = np.empty(n, np.int32)
        st = OutlierStats()
        _check(self.lib.sf_map_radius_outliers(self.h, C.c_double(radius), C.c_int(int(min_neighbors)), _p(keep), _p(cnt), C.byref(st)))
        return keep.astype(bool), cnt, st.as_dict()

    def compute_fpfh(self, radius, orient="none", toward=(0, 0, 1), profile=False):
        """sf_map_compute_fpfh (pcl::FPFHEstimation, Open3D compute_fpfh_feature): the 33-bin FPFH of every map point from the points with
        float32 d2 < float32(radius^2) and the map's normals -> (Features in original point order, stats dict).  orient "none": the
        normals as stored; "direction": negated when n . toward < 0; "viewpoint": negated when n . (toward - x) < 0.  A point without a
        normal or without a usable pair gets 33 zeros and valid = 0."""
        p, st, out = _fpfh_params(radius, orient, toward, profile), FpfhStats(), Features(self.ctx)
        _check(self.lib.sf_map_compute_fpfh(self.h, C.byref(p), out.h, C.byref(st)))
        return out, st.as_dict()

    def compute_spfh(self, radius, orient="none", toward=(0, 0, 1)):
        """sf_map_compute_spfh: the integer half of compute_fpfh -> (counts uint32 [n, 33], n_pairs int32 [n]), original point order;
        SPFH_i = counts_i * (100 / n_pairs_i)."""
        n = len(self)
        p = _fpfh_params(radius, orient, toward, False)
        counts, pairs = np.zeros((n, FPFH_DIM), np.uint32), np.zeros(n, np.int32)
        _check(self.lib.sf_map_compute_spfh(self.h, C.byref(p), _p(counts), _p(pairs)))
        return counts, pairs

    def iss_saliency(self, salient_radius, non_max_radius=None, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, min_lambda3=0.0):
        """sf_map_iss_saliency: the first pass of iss_keypoints -> dict(lambda float64 [n, 3] descending, n_neighbors int32 [n] (the
        count of radius_outliers at salient_radius), salient bool [n]), original point order; zeros for points that are not indexed.
        non_max_radius plays no part in it (None: the salient radius stands in, the parameters are checked together)."""
        n = len(self)
        p = _iss_params(salient_radius, salient_radius if non_max_radius is None else non_max_radius, gamma_21, gamma_32, min_neighbors, min_lambda3, False)
        lam, cnt, sal = np.zeros((n, 3), np.float64), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        _check(self.lib.sf_map_iss_saliency(self.h, C.byref(p), _p(lam), _p(cnt), _p(sal)))
        return {"lambda": lam, "n_neighbors": cnt, "salient": sal.astype(bool)}

    def iss_keypoints(self, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, min_lambda3=0.0, profile=False):
        """sf_map_iss_keypoints (Open3D compute_iss_keypoints, the unweighted pcl::ISSKeypoint3D): a point is salient when the
        eigenvalues of the covariance of its neighbours within salient_radius have lambda2 < gamma_21 lambda1, lambda3 < gamma_32
        lambda2 and lambda3 > min_lambda3 (an absolute floor in m^2), and a keypoint when no salient point within non_max_radius has a
        larger lambda3 (ties: the smallest index) -> dict(indices int32 [k] ascending, flags bool [n], stats), original point order."""
        n = len(self)
        p, st, nk = _iss_params(salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors, min_lambda3, profile), IssStats(), C.c_int64()
        idx, flags = np.zeros(max(n, 1), np.int32), np.zeros(n, np.uint8)
        _check(self.lib.sf_map_iss_keypoints(self.h, C.byref(p), _p(idx), C.c_int64(n), C.byref(nk), _p(flags), C.byref(st)))
        return dict(indices=idx[:nk.value].copy(), flags=flags.astype(bool), stats=st.as_dict())

    def _clusters(self, call, *args):
        n = len(self)
        labels = np.empty(n, np.int32)
        sizes = np.empty(max(n, 1), np.int32)                      # (there are at most n clusters)
        st = ClusterStats()
        _check(call(self.h, *args, _p(labels), _p(sizes), C.c_int64(len(sizes)), C.byref(st)))
        return labels, sizes[:int(st.n_clusters)].copy(), st.as_dict()

    def cluster_dbscan(self, eps, min_points):
        """sf_map_cluster_dbscan (Open3D cluster_dbscan, scikit-learn DBSCAN): -> (labels int32 [n], sizes int32 [C], stats dict), original
        point order.  A point is core when `min_points` indexed points, itself included, lie within eps (float32 d2 < float32(eps^2));
        clusters are numbered by their smallest core point; a border point takes the smallest label among its core neighbours; -1: noise."""
        return self._clusters(self.lib.sf_map_cluster_dbscan, C.c_double(eps), C.c_int(int(min_points)))

    def cluster_euclidean(self, tolerance, min_size=1, max_size=0):
        """sf_map_cluster_euclidean (pcl::EuclideanClusterExtraction): the connected pieces at `tolerance`, those with fewer than min_size
        or more than max_size (> 0) points labelled -1, the others numbered by their smallest point -> (labels, sizes, stats dict)."""
        return self._clusters(self.lib.sf_map_cluster_euclidean, C.c_double(tolerance), C.c_int64(int(min_size)), C.c_int64(int(max_size)))

    def build_neighbour_table(self):
        """sf_map_build_neighbour_table: per indexed point its up to 7 nearest other points and a radius free of any further
        point (include/slamfusion.h); kept until build / patch move the points."""
        _check(self.lib.sf_map_build_neighbour_table(self.h))
        return self

    def set_neighbour_table(self, mode="auto"):
        """sf_map_set_neighbour_table: "never", "auto" (default) or "always"."""
        _check(self.lib.sf_map_set_neighbour_table(self.h, C.c_int({"never": 0, "auto": 1, "always": 2}[mode])))
        return self

    def neighbour_table_info(self):
        """sf_map_neighbour_table_info -> dict(present, entries, bytes, build_ms); build_ms is -1 unless profile_launches was on."""
        a = (C.c_int64 * 4)()
        _check(self.lib.sf_map_neighbour_table_info(self.h, a))
        return {"present": bool(a[0]), "entries": a[1], "bytes": a[2], "build_ms": a[3]}

    def download_neighbour_table(self):
        """The table as it lies on the device: (ids [n, 7] uint32 sorted positions, 0xffffffff = none; r [n] float32)."""
        info = self.neighbour_table_info()
        raw = np.zeros((max(info["entries"], 1), 8), np.uint32)
        n = C.c_int64()
        _check(self.lib.sf_map_download_neighbour_table(self.h, _p(raw), C.c_int64(len(raw)), C.byref(n)))
        raw = raw[:n.value]
        return raw[:, :7].copy(), raw[:, 7].copy().view(np.float32)

    def nn_seeded(self, queries, seed_pos, max_d2=np.inf):
        """sf_map_nn_seeded: the table look-up alone, from the indexed point at SORTED position seed_pos[i] (-1: none) ->
        (idx, d2, served); served rows equal nn() bit for bit, the others are -1 / inf."""
        q = _f32(queries).reshape(-1, 3)
        s = np.ascontiguousarray(seed_pos, dtype=np.int32).reshape(-1)
        assert len(s) == len(q)
        idx = np.empty(len(q), np.int32)
        d2 = np.empty(len(q), np.float32)
        served = np.empty(len(q), np.uint8)
        _check(self.lib.sf_map_nn_seeded(self.h, _p(q), C.c_int64(len(q)), _p(s), C.c_float(min(max_d2, 3.0e38)), _p(idx), _p(d2), _p(served)))
        return idx, d2, served.astype(bool)

    def download_nearest_gap(self):
        """sf_map_download_nearest_gap: the nearest gap of every indexed point, [n] float32 in sorted order."""
        gap = np.zeros(max(self.neighbour_table_info()["entries"], 1), np.float32)
        n = C.c_int64()
        _check(self.lib.sf_map_download_nearest_gap(self.h, _p(gap), C.c_int64(len(gap)), C.byref(n)))
        return gap[:n.value].copy()

    def nn_seeded_stages(self, queries, seed_pos, max_d2=np.inf):
        """sf_map_nn_seeded_stages -> (idx, d2, stage, lb2): nn_seeded with the stage that served each query (0 not served,
        1 the nearest gap alone, 2 the table) and the squared runner-up bound it left."""
        q = _f32(queries).reshape(-1, 3)
        s = np.ascontiguousarray(seed_pos, dtype=np.int32).reshape(-1)
        assert len(s) == len(q)
        idx = np.empty(len(q), np.int32)
        d2 = np.empty(len(q), np.float32)
        stage = np.empty(len(q), np.uint8)
        lb2 = np.empty(len(q), np.float32)
        _check(self.lib.sf_map_nn_seeded_stages(self.h, _p(q), C.c_int64(len(q)), _p(s), C.c_float(min(max_d2, 3.0e38)), _p(idx), _p(d2), _p(stage), _p(lb2)))
        return idx, d2, stage, lb2

    def visibility(self, image, pose, half_cols=1, half_rows=1, min_hits=1, range_margin=0.2, range_ratio=0.01, profile=False):
        """sf_map_visibility: every point's class (VIS_CLASSES) against one RangeImage built from a scan taken at `pose` (map <-
        sensor, [4, 4]; None: the identity) -> (cls uint8 [n] in the original point order, stats dict).  The map stays as it is."""
        p, st, cls = _visibility_params(half_cols, half_rows, min_hits, range_margin, range_ratio, profile), VisibilityStats(), np.zeros(max(len(self), 1), np.uint8)
        pose = None if pose is None else _f64(pose).reshape(16)
        _check(self.lib.sf_map_visibility(self.h, image.h, _p(pose) if pose is not None else None, C.byref(p), _p(cls), C.byref(st)))
        return cls[:len(self)], st.as_dict()

    def visibility_votes(self, images, poses, half_cols=1, half_rows=1, min_hits=1, range_margin=0.2, range_ratio=0.01, profile=False):
        """sf_map_visibility_votes: per point the number of the images (up to 64 RangeImage objects, poses [B, 4, 4]) that class it
        SEEN_THROUGH and WITHIN, in one pass over the map -> (seen_through uint16 [n], within uint16 [n], stats dict)."""
        handles, poses, b = _images_and_poses(images, poses)
        p, st, n = _visibility_params(half_cols, half_rows, min_hits, range_margin, range_ratio, profile), VisibilityStats(), len(self)
        seen, within = np.zeros(max(n, 1), np.uint16), np.zeros(max(n, 1), np.uint16)
        _check(self.lib.sf_map_visibility_votes(self.h, handles, _p(poses) if poses is not None else None, C.c_int64(b), C.byref(p), _p(seen), _p(within), C.byref(st)))
        return seen[:n], within[:n], st.as_dict()

    def profile_launches(self, on=True):
        """sf_map_profile_launches: device events around the kernel launches of nn / knn / estimate_normals*."""
        _check(self.lib.sf_map_profile_launches(self.h, C.c_int(int(bool(on)))))
        return self

    def last_launch_ms(self):
        ms = C.c_float()
        _check(self.lib.sf_map_last_launch_ms(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            self.lib.sf_map_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Features:
    """sf_features: n descriptor rows of 33 float32 and a validity byte per row on the device, in the point order of what produced
    them (Map.compute_fpfh, Cloud.compute_fpfh, or `upload`)."""

    def __init__(self, ctx, rows=None, valid=None):
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p()
        _check(self.lib.sf_features_create(ctx.h, C.byref(self.h)))
        _live.add(self)
        if rows is not None:
            self.upload(rows, valid)

    def upload(self, rows, valid=None):
        """rows [n, 33] float32; valid [n] (None: all offered as valid).  A row holding a non-finite value is invalid either way."""
        rows = _f32(rows).reshape(-1, FPFH_DIM)
        v = None
        if valid is not None:
            v = np.ascontiguousarray(np.asarray(valid).reshape(-1) != 0, dtype=np.uint8)
            if len(v) != len(rows):
                raise SlamFusionError("valid must have one entry per row (%d, got %d)" % (len(rows), len(v)))
        _check(self.lib.sf_features_upload(self.h, _p(rows), _p(v) if v is not None else None, C.c_int64(len(rows))))
        return self

    def __len__(self):
        n = C.c_int64()
        _check(self.lib.sf_features_size(self.h, C.byref(n)))
        return n.value

    def download(self):
        """-> (rows float32 [n, 33], valid bool [n])"""
        n = len(self)
        rows, valid = np.zeros((n, FPFH_DIM), np.float32), np.zeros(n, np.uint8)
        _check(self.lib.sf_features_download(self.h, _p(rows), _p(valid), C.c_int64(n), None))
        return rows, valid.astype(bool)

    def gather(self, indices):
        """sf_features_gather: -> a new Features whose row r is row indices[r] of this set with its validity, in the order given
        (repeats allowed): the descriptors of chosen points, e.g. of Map.iss_keypoints."""
        rows, out = _rows(indices), Features(self.ctx)
        _check(self.lib.sf_features_gather(self.h, _p(rows) if len(rows) else None, C.c_int64(len(rows)), out.h))
        return out

    def match(self, other, ratio=0, mutual=False, max_pairs=None, profile=False):
        """sf_features_match: for every valid row the valid row of `other` with the smallest float32 squared distance (ties: the
        smallest index) -> dict(idx int32 [n] (-1: none), dist2, second2 float32 [n], pairs int32 [m, 2], stats).  pairs are the
        accepted (i, idx[i]) in ascending i: idx >= 0, with 0 < ratio < 1 also dist2 < float32(ratio^2) * second2 (Lowe's test), with
        `mutual` also i being the best row of this set for other[idx[i]]; at most max_pairs of them (None: all), stats counts all."""
        if not isinstance(other, Features):
            raise SlamFusionError("match: the other side must be a Features object")
        n = len(self)
        cap = n if max_pairs is None else max(int(max_pairs), 0)
        p, st = MatchParams(float(ratio), int(bool(mutual)), int(bool(profile))), MatchStats()
        idx, d2, s2 = np.full(n, -1, np.int32), np.full(n, np.inf, np.float32), np.full(n, np.inf, np.float32)
        pairs = np.zeros((max(cap, 1), 2), np.int32)
        _check(self.lib.sf_features_match(self.h, other.h, C.byref(p), _p(idx), _p(d2), _p(s2), _p(pairs), C.c_int64(cap), C.byref(st)))
        return dict(idx=idx, dist2=d2, second2=s2, pairs=pairs[:min(int(st.n_matched), cap)].copy(), stats=st.as_dict())

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.sf_features_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RangeImage:
    """sf_range_image: an azimuth x elevation range image on the device (include/slamfusion.h): per pixel the
    smallest range of the points that fall into it and the index of that point.  el_min / el_max in radians (default -25 .. +3
    degrees)."""

    def __init__(self, ctx, width=2048, height=64, el_min=None, el_max=None, min_range=0.5, max_range=120.0):
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p()
        p = RangeImageParams()
        self.lib.sf_range_image_default_params(C.byref(p))
        p.width, p.height, p.min_range, p.max_range = int(width), int(height), float(min_range), float(max_range)
        if el_min is not None:
            p.el_min = float(el_min)
        if el_max is not None:
            p.el_max = float(el_max)
        _check(self.lib.sf_range_image_create(ctx.h, C.byref(p), C.byref(self.h)))
        _live.add(self)

    @property
    def params(self):
        p = RangeImageParams()
        _check(self.lib.sf_range_image_info(self.h, C.byref(p)))
        return p.as_dict()

    def build(self, cloud, pose=None):
        """sf_range_image_build: the image of `cloud` seen from `pose` ([4, 4] parent <- sensor; None: the cloud is in the sensor
        frame already), replacing what the image held -> stats dict."""
        st = RangeImageStats()
        pose = None if pose is None else _f64(pose).reshape(16)
        _check(self.lib.sf_range_image_build(self.h, cloud.h, _p(pose) if pose is not None else None, C.byref(st)))
        return st.as_dict()

    def download(self):
        """-> (range float32 [H, W], +inf where empty; index int32 [H, W], -1 where empty)"""
        q = self.params
        rng, idx = np.empty((q["height"], q["width"]), np.float32), np.empty((q["height"], q["width"]), np.int32)
        _check(self.lib.sf_range_image_download(self.h, _p(rng), _p(idx)))
        return rng, idx

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.sf_range_image_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PlaceDB:
    """sf_place_db: a database of Scan Context descriptors with the poses of the keyframes they were built from, on the device
    (include/slamfusion.h).  params: num_rings, num_sectors, min_range, max_range, sensor_height.  A query is
    matched against every entry under every column shift; the best shift is the yaw between the two."""

    def __init__(self, ctx, **params):
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p()
        p = _scan_context_params(**params)
        _check(self.lib.sf_place_db_create(ctx.h, C.byref(p), C.byref(self.h)))
        _live.add(self)

    @property
    def params(self):
        p = ScanContextParams()
        _check(self.lib.sf_place_db_info(self.h, C.byref(p), None))
        return p.as_dict()

    @property
    def shape(self):
        q = self.params
        return q["num_rings"], q["num_sectors"]

    def __len__(self):
        n = C.c_int64()
        _check(self.lib.sf_place_db_info(self.h, None, C.byref(n)))
        return int(n.value)

    def clear(self):
        _check(self.lib.sf_place_db_clear(self.h))

    def add(self, cloud, entry_pose, pose=None):
        """sf_place_db_add_cloud: the descriptor of `cloud` (seen from `pose`, None: already in the sensor frame) appended with the
        keyframe's pose entry_pose ([4, 4] map <- sensor) -> (the entry's index, stats dict)."""
        st, index = ScanContextStats(), C.c_int64()
        pose = None if pose is None else _f64(pose).reshape(16)
        entry_pose = None if entry_pose is None else _f64(entry_pose).reshape(16)
        _check(self.lib.sf_place_db_add_cloud(self.h, cloud.h, _p(pose) if pose is not None else None, _p(entry_pose) if entry_pose is not None else None,
                                              C.byref(index), C.byref(st)))
        return int(index.value), st.as_dict()

    def _rows(self, desc):
        desc = _f32(desc)
        rows = desc.reshape((-1,) + self.shape)
        return rows, len(rows)

    def add_descriptors(self, desc, poses=None):
        """sf_place_db_add_descriptors: stored rows (float32 [n, num_rings, num_sectors]) and their poses ([n, 4, 4]; None: identities)"""
        rows, n = self._rows(desc)
        if poses is not None:
            poses = _f64(poses).reshape(-1, 16)
            if len(poses) != n:
                raise SlamFusionError("one pose per descriptor (%d descriptors, %d poses)" % (n, len(poses)))
        _check(self.lib.sf_place_db_add_descriptors(self.h, _p(rows), _p(poses) if poses is not None else None, C.c_int64(n)))

    def download(self):
        """-> (descriptors float32 [n, num_rings, num_sectors], poses float64 [n, 4, 4])"""
        n = len(self)
        desc, poses, got = np.zeros((n,) + self.shape, np.float32), np.zeros((n, 4, 4)), C.c_int64()
        _check(self.lib.sf_place_db_download(self.h, _p(desc), _p(poses), C.c_int64(n), C.byref(got)))
        return desc, poses

    def distances(self, queries):
        """sf_place_db_distances: queries float32 [Q, num_rings, num_sectors] (or one descriptor) ->
        (D float64 [Q, n], shift int32 [Q, n], stats dict)"""
        rows, q = self._rows(queries)
        n, st = len(self), PlaceMatchStats()
        dist, shift = np.zeros((q, n)), np.zeros((q, n), np.int32)
        _check(self.lib.sf_place_db_distances(self.h, _p(rows), C.c_int64(q), _p(dist), _p(shift), C.byref(st)))
        return dist, shift, st.as_dict()

    def query(self, queries, k):
        """sf_place_db_query: per query the k entries with the smallest (D, index) -> dict(idx int32 [Q, k] (-1: no entry), dist float64
        [Q, k] (+inf there), shift int32 [Q, k], poses float64 [Q, k, 4, 4]: T_entry . Rz(shift 2 pi / num_sectors), stats)"""
        rows, q = self._rows(queries)
        kk, st = max(int(k), 1), PlaceMatchStats()
        idx, dist, shift, poses = np.zeros((q, kk), np.int32), np.zeros((q, kk)), np.zeros((q, kk), np.int32), np.zeros((q, kk, 4, 4))
        _check(self.lib.sf_place_db_query(self.h, _p(rows), C.c_int64(q), C.c_int(int(k)), _p(idx), _p(dist), _p(shift), _p(poses), C.byref(st)))
        return dict(idx=idx, dist=dist, shift=shift, poses=poses, stats=st.as_dict())

    def query_cloud(self, cloud, k, pose=None):
        """sf_place_db_query_cloud: the same for one cloud, whose descriptor is built and matched on the device -> the dict of `query`
        with Q = 1 and build_stats, the statistics of the descriptor build"""
        kk, st, bst = max(int(k), 1), PlaceMatchStats(), ScanContextStats()
        idx, dist, shift, poses = np.zeros((1, kk), np.int32), np.zeros((1, kk)), np.zeros((1, kk), np.int32), np.zeros((1, kk, 4, 4))
        pose = None if pose is None else _f64(pose).reshape(16)
        _check(self.lib.sf_place_db_query_cloud(self.h, cloud.h, _p(pose) if pose is not None else None, C.c_int(int(k)), _p(idx), _p(dist), _p(shift), _p(poses),
                                                C.byref(st), C.byref(bst)))
        return dict(idx=idx, dist=dist, shift=shift, poses=poses, stats=st.as_dict(), build_stats=bst.as_dict())

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.sf_place_db_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Ndt:
    """sf_ndt: Normal Distributions Transform registration of scans against the per-voxel Gaussians of `target` (a Cloud or a Map)
    at cell = resolution (include/slamfusion.h).  neighbours: 1 (the home cell) or 7 (plus the face neighbours)."""

    def __init__(self, ctx, target, resolution, neighbours=7, outlier_ratio=0.55, min_points=6, min_eig_ratio=0.01, step_size=0.1,
                 transformation_epsilon=1e-4, max_iterations=30, hessian_floor=1e-6, profile=False):
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p()
        p = NdtParams()
        self.lib.sf_ndt_default_params(C.byref(p))
        p.resolution, p.outlier_ratio, p.step_size, p.transformation_epsilon = float(resolution), float(outlier_ratio), float(step_size), float(transformation_epsilon)
        p.min_eig_ratio, p.hessian_floor = float(min_eig_ratio), float(hessian_floor)
        p.min_points, p.neighbours, p.max_iterations, p.profile = int(min_points), int(neighbours), int(max_iterations), int(bool(profile))
        self.params = p
        _check(self.lib.sf_ndt_create(ctx.h, C.byref(p), C.byref(self.h)))
        _live.add(self)
        self.batch = 0
        if target is not None:
            self.set_target(target)

    def set_target(self, target):
        if isinstance(target, Map):
            _check(self.lib.sf_ndt_set_target_map(self.h, target.h))
        elif isinstance(target, Cloud):
            _check(self.lib.sf_ndt_set_target_cloud(self.h, target.h))
        else:
            raise SlamFusionError("Ndt: the target must be a Cloud or a Map")
        return self

    def voxels(self):
        """-> dict(cell int64 [n] ascending, count int32 [n], mean [n, 3], cov [n, 6], icov [n, 6] (xx xy xz yy yz zz), dims)"""
        n = C.c_int64()
        _check(self.lib.sf_ndt_download_voxels(self.h, None, None, None, None, None, C.c_int64(0), C.byref(n)))
        n = n.value
        cell, count = np.zeros(n, np.int64), np.zeros(n, np.int32)
        mean, cov, icov = np.zeros((n, 3), np.float64), np.zeros((n, 6), np.float64), np.zeros((n, 6), np.float64)
        if n:
            _check(self.lib.sf_ndt_download_voxels(self.h, _p(cell), _p(count), _p(mean), _p(cov), _p(icov), C.c_int64(n), None))
        return dict(cell=cell, count=count, mean=mean, cov=cov, icov=icov, dims=self.stats()["dims"])

    def _set_source(self, source):
        if isinstance(source, Cloud):
            _check(self.lib.sf_ndt_set_source_cloud(self.h, source.h))
            self.batch = 1
            return
        xyz = _f32(source)
        if xyz.ndim != 3:
            xyz = xyz.reshape(1, -1, 3)
        _check(self.lib.sf_ndt_set_source_batch(self.h, _p(xyz) if xyz.size else None, C.c_int64(xyz.shape[1]), C.c_int(xyz.shape[0])))
        self.batch = xyz.shape[0]

    def derivatives(self, source, poses):
        """Score, gradient and Hessian of `source` (a Cloud or [n, 3]) at poses [k, 4, 4] -> a list of k dicts."""
        self._set_source(source)
        poses = _f64(poses).reshape(-1, 16)
        out = (NdtResult * max(len(poses), 1))()
        _check(self.lib.sf_ndt_derivatives(self.h, _p(poses) if len(poses) else None, C.c_int64(len(poses)), out))
        return [out[i].as_dict() for i in range(len(poses))]

    def align(self, source, init=None, trace=False):
        """One scan from `init` (None: the identity) -> dict(T64, score, gradient, hessian, n_inside, n_terms, iterations, converged,
        modified, flags[, trace [iterations + 1, 4, 4]])."""
        self._set_source(source)
        init = _f64(np.eye(4) if init is None else init).reshape(16)
        out = NdtResult()
        tr = np.zeros((int(self.params.max_iterations) + 1, 16), np.float64) if trace else None
        _check(self.lib.sf_ndt_align(self.h, _p(init), C.byref(out), _p(tr) if trace else None))
        r = out.as_dict()
        if trace:
            r["trace"] = tr[:r["iterations"] + 1].reshape(-1, 4, 4).copy()
        return r

    def align_batch(self, sources, inits):
        """sources [batch, n, 3] from inits [batch, 4, 4] -> a list of batch dicts; entry b is bit for bit align(sources[b], inits[b])."""
        self._set_source(_f32(sources).reshape(len(sources), -1, 3))
        inits = _f64(inits).reshape(-1, 16)
        if len(inits) != self.batch:
            raise SlamFusionError("align_batch: %d poses for %d scans" % (len(inits), self.batch))
        out = (NdtResult * self.batch)()
        _check(self.lib.sf_ndt_align_batch(self.h, _p(inits), out))
        return [out[i].as_dict() for i in range(self.batch)]

    def stats(self):
        st = NdtStats()
        _check(self.lib.sf_ndt_stats_read(self.h, C.byref(st)))
        return st.as_dict()

    def set_line_search(self, trials=8, step_max=1.0, armijo=1e-4):
        """The backtracking line search of the alignments from now on: per iteration the `trials` step lengths
        alpha_max / 2^k along the unscaled Newton direction, alpha_max = min(1, step_max / |d|), the first that meets the Armijo
        condition taken.  trials=0 switches it off: the alignments are then bit for bit those of an object that never had it."""
        p = NdtLineSearch(int(trials), 0, float(step_max), float(armijo))
        _check(self.lib.sf_ndt_set_line_search(self.h, C.byref(p)))
        return self

    def scores(self, source, poses):
        """Score and number of terms of `source` (a Cloud or [n, 3]) at poses [k, 4, 4] -> (score float64 [k], n_terms int64 [k]): bit for
        bit the score and n_terms of derivatives() there, without the gradient and the Hessian."""
        self._set_source(source)
        poses = _f64(poses).reshape(-1, 16)
        score, terms = np.zeros(len(poses), np.float64), np.zeros(len(poses), np.int64)
        _check(self.lib.sf_ndt_scores(self.h, _p(poses) if len(poses) else None, C.c_int64(len(poses)), _p(score) if len(poses) else None,
                                      _p(terms) if len(poses) else None))
        return score, terms

    def line_search_rows(self):
        """The line search of the last align() with the search on, one dict per evaluated iteration (NdtLsRow.as_dict)."""
        n = C.c_int64()
        _check(self.lib.sf_ndt_line_search_read(self.h, None, C.c_int64(0), C.byref(n)))
        rows = (NdtLsRow * max(n.value, 1))()
        _check(self.lib.sf_ndt_line_search_read(self.h, rows, C.c_int64(n.value), None))
        return [rows[i].as_dict() for i in range(n.value)]

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.sf_ndt_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NdtPyramid:
    """Coarse-to-fine NDT (sf_ndt_align_levels): one Ndt per entry of `resolutions` (descending) on the same target,
    aligned in turn, each level from the pose where the previous one ended.  line_search: True (the defaults of
    Ndt.set_line_search), False, or a dict of its arguments; ndt_kwargs go to every Ndt."""

    def __init__(self, ctx, target, resolutions, line_search=True, **ndt_kwargs):
        self.ctx, self.lib = ctx, ctx.lib
        self.levels = []
        _live.add(self)
        for r in resolutions:
            self.levels.append(Ndt(ctx, target, float(r), **ndt_kwargs))
            if line_search:
                self.levels[-1].set_line_search(**(line_search if isinstance(line_search, dict) else {}))
        if not self.levels:
            raise SlamFusionError("NdtPyramid: no resolutions")

    def _run(self, sources, inits):
        for lv in self.levels:
            lv._set_source(sources)
        batch = self.levels[0].batch
        inits = _f64(inits).reshape(-1, 16)
        if len(inits) != batch:
            raise SlamFusionError("NdtPyramid: %d poses for %d scans" % (len(inits), batch))
        n = len(self.levels)
        handles = (C.c_void_p * n)(*[lv.h.value for lv in self.levels])
        out, per = (NdtResult * batch)(), (NdtResult * (n * batch))()
        _check(self.lib.sf_ndt_align_levels(handles, C.c_int(n), _p(inits), out, per))
        res = [out[b].as_dict() for b in range(batch)]
        for b in range(batch):
            res[b]["per_level"] = [per[l * batch + b].as_dict() for l in range(n)]
        return res

    def align(self, source, init=None):
        """One scan (a Cloud or [n, 3]) from `init` (None: the identity) -> the last level's dict of Ndt.align plus per_level (a list of
        every level's dict)."""
        return self._run(source if isinstance(source, Cloud) else _f32(source).reshape(1, -1, 3), np.eye(4) if init is None else init)[0]

    def align_batch(self, sources, inits):
        """sources [batch, n, 3] from inits [batch, 4, 4] -> a list of batch such dicts."""
        return self._run(_f32(sources).reshape(len(sources), -1, 3), inits)

    def close(self):
        for lv in getattr(self, "levels", []):
            lv.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Icp:
    """sf_icp: mirrors ICPPointToPoint (icp_point_to_point.h:41-136) setter for setter."""

    def __init__(self, ctx, max_correspondence_dist=0.5, num_iterations=10,
                 acceptable_mean_error=0.05, transformation_epsilon=1e-5):
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p()
        self._map = None
        self.batch = 1
        _check(self.lib.sf_icp_create(ctx.h, C.c_float(max_correspondence_dist), C.c_int(num_iterations),
                                      C.c_float(acceptable_mean_error), C.c_float(transformation_epsilon),
                                      C.byref(self.h)))
        _live.add(self)

    def set_max_correspondence_dist(self, v):
        _check(self.lib.sf_icp_set_max_correspondence_dist(self.h, C.c_float(v)))

    def set_num_iterations(self, v):
        _check(self.lib.sf_icp_set_num_iterations(self.h, C.c_int(v)))

    def set_transformation_epsilon(self, v):
        _check(self.lib.sf_icp_set_transformation_epsilon(self.h, C.c_float(v)))

    def set_acceptable_mean_error(self, v):
        _check(self.lib.sf_icp_set_acceptable_mean_error(self.h, C.c_float(v)))

    def set_debug_mode(self, on):
        _check(self.lib.sf_icp_set_debug_mode(self.h, C.c_int(int(on))))

    def set_initial_transformation(self, T):
        T = np.asarray(T)
        if T.dtype == np.float32:
            T = _f32(T).reshape(16)
            _check(self.lib.sf_icp_set_initial_transformation(self.h, _p(T)))
        else:
            T = _f64(T).reshape(16)
            _check(self.lib.sf_icp_set_initial_transformation_f64(self.h, _p(T)))

    def set_source(self, xyz):
        if isinstance(xyz, Cloud):
            _check(self.lib.sf_icp_set_source_cloud(self.h, xyz.h))
        else:
            xyz = _f32(xyz).reshape(-1, 3)
            _check(self.lib.sf_icp_set_source(self.h, _p(xyz), C.c_int64(len(xyz))))
        self.batch = 1

    def set_source_batch(self, xyz):
        xyz = _f32(xyz)
        assert xyz.ndim == 3 and xyz.shape[2] == 3
        _check(self.lib.sf_icp_set_source_batch(self.h, _p(xyz), C.c_int64(xyz.shape[1]), C.c_int(xyz.shape[0])))
        self.batch = xyz.shape[0]

    def set_source_batch_host_ptr(self, ptr, n_per_scan, batch):
        """batch x n_per_scan x 3 float32 at a raw HOST address (e.g. pinned memory: the copy is then asynchronous).  With the
        pipeline on, a buffer set while an alignment is unfetched is read on an internal stream: it is free again only once that
        batch's alignment has been fetched; otherwise once the context's stream has passed it (include/slamfusion.h)"""
        _check(self.lib.sf_icp_set_source_batch(self.h, C.c_void_p(ptr), C.c_int64(n_per_scan), C.c_int(batch)))
        self.batch = batch

    def set_source_batch_device(self, ptr, n_per_scan, batch):
        _check(self.lib.sf_icp_set_source_batch_device(self.h, C.c_void_p(ptr), C.c_int64(n_per_scan), C.c_int(batch)))
        self.batch = batch

    def set_initial_batch(self, inits=None):
        if inits is None:
            _check(self.lib.sf_icp_set_initial_batch_f64(self.h, None))
        else:
            inits = _f64(inits).reshape(self.batch, 16)
            _check(self.lib.sf_icp_set_initial_batch_f64(self.h, _p(inits)))

    def set_target(self, target):
        if isinstance(target, Map):
            self._map = target
            _check(self.lib.sf_icp_set_target_map(self.h, target.h))
        else:
            xyz = _f32(target).reshape(-1, 3)
            _check(self.lib.sf_icp_set_target(self.h, _p(xyz), C.c_int64(len(xyz))))

    def use_graph(self, on=True):
        _check(self.lib.sf_icp_use_graph(self.h, C.c_int(int(on))))

    def graph_counts(self):
        a, b = C.c_int64(), C.c_int64()
        _check(self.lib.sf_icp_graph_counts(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_source_scan(self, raw_cloud, stride, center, radius):
        """sf_icp_set_source_scan: subsample + radius crop + set_source in one pass, the count stays on the device"""
        c = _f32(center)
        _check(self.lib.sf_icp_set_source_scan(self.h, raw_cloud.h, C.c_int(int(stride)), _p(c), C.c_double(radius)))
        self.batch = 1

    def source_count(self):
        n = C.c_int64()
        _check(self.lib.sf_icp_source_count(self.h, C.byref(n)))
        return n.value

    def set_fused(self, on=True):
        _check(self.lib.sf_icp_set_fused(self.h, C.c_int(int(on))))

    def fused_count(self):
        a = C.c_int64()
        _check(self.lib.sf_icp_fused_count(self.h, C.byref(a)))
        return a.value

    def fused_redone(self):
        n = C.c_int64()
        _check(self.lib.sf_icp_fused_redone(self.h, C.byref(n)))
        return n.value

    def test_inject_barrier_timeout(self):
        _check(self.lib.sf_icp_test_inject_barrier_timeout(self.h))

    def test_download_cache(self, b=0):
        """Test hook (sf_icp_test_download_cache): the neighbour cache of scan b as the launch list of the latest alignment left it,
        read only.  -> dict: x0 [n][3] (the query's source point), orig [n] (its index in the scan as given, -1 where the ordering
        kept none), nbr [n][3], j [n] (index position, negative: none), e [n], and T (4x4), motion, cache_live, n_research,
        iterations, mode, batch, ordered of the scan's state."""
        info = IcpCacheInfo()
        _check(self.lib.sf_icp_test_download_cache(self.h, int(b), 0, None, None, None, None, None, C.addressof(info)))
        n = int(info.n)
        x0, nbr = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        orig, j, e = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float32)
        _check(self.lib.sf_icp_test_download_cache(self.h, int(b), n, _p(x0), _p(orig), _p(nbr), _p(j), _p(e), C.addressof(info)))
        return dict(x0=x0, orig=orig, nbr=nbr, j=j, e=e, T=np.array(info.T[:], np.float64).reshape(4, 4), motion=float(info.motion), n=n, batch=info.batch, mode=info.mode,
                    cache_live=info.cache_live, n_research=info.n_research, iterations=info.iterations, ordered=info.ordered)

    def set_nn_reuse(self, on=True):
        _check(self.lib.sf_icp_set_nn_reuse(self.h, C.c_int(int(on))))

    def set_freeze(self, on="auto"):
        """Frozen pairs (sf_icp_set_freeze): P2PLANE launch list of wide scans, see include/slamfusion.h.
        False / "off", "auto" (default: batches of at least 0.7 M queries), True / "always"."""
        code = {False: 0, "off": 0, "auto": 1, True: 2, "always": 2}[on]
        _check(self.lib.sf_icp_set_freeze(self.h, C.c_int(code)))

    def set_robust_kernel(self, kind="none", k=None):
        """Robust M-estimator kernel of point-to-plane ICP (sf_icp_set_robust_kernel; REF_CPP and O3D_P2P ignore it), see
        include/slamfusion.h.  "none" (default), "huber", "cauchy", "tukey" or "gm" (Geman-McClure), scale k in metres
        (finite, > 0; ignored for "none").  Each pair's JtJ / Jtr terms are weighted by w(r) of its plane residual; fitness,
        rmse and n_corr stay unweighted.  P2PLANE does not freeze or take the tile search while a kind is set."""
        code = ROBUST_KINDS[kind]
        _check(self.lib.sf_icp_set_robust_kernel(self.h, code, float("nan") if k is None and code != 0 else float(k or 0.0)))

    def set_covariance(self, on=True, sensor_sigma=0.0):
        """Pose covariance and degeneracy of every alignment from now on (sf_icp_set_covariance, include/slamfusion.h): one more
        evaluation of the mode's objective at the final pose, enqueued behind the last iteration.  sensor_sigma (metres) > 0
        scales the covariance; 0 uses the residual variance the pairs themselves show.  Default off."""
        _check(self.lib.sf_icp_set_covariance(self.h, int(bool(on)), float(sensor_sigma)))

    def set_degeneracy_thresholds(self, trans=0.0, rot=0.0, inflate_trans_var=0.0, inflate_rot_var=0.0):
        """Eigenvalues of the marginal translation / rotation information divided by the weight sum below these thresholds
        flag the alignment (COV_FLAGS) and add inflate_* (m^2, rad^2) to cov along every flagged eigenvector.  0 = never."""
        _check(self.lib.sf_icp_set_degeneracy_thresholds(self.h, float(trans), float(rot), float(inflate_trans_var), float(inflate_rot_var)))

    def fetch_covariance(self, previous=False, batch=None):
        """One dict per scan (6x6 numpy info / cov, sigma2, sigma2_hat, weight_sum, trans_info, trans_dir, rot_info, rot_dir,
        n_corr, flags) of the alignment fetch_results last returned, or with previous=True of the one fetch_previous returns."""
        if previous:
            arr = (IcpCovariance * int(batch or getattr(self, "_prev_batch", None) or self.batch))()
            _check(self.lib.sf_icp_fetch_covariance_previous(self.h, arr))
        else:
            arr = (IcpCovariance * int(batch or getattr(self, "_last_batch", None) or self.batch))()
            _check(self.lib.sf_icp_fetch_covariance(self.h, arr))
        return [c.as_dict() for c in arr]

    def set_wide_scan_points(self, points):
        """Scans above this many points take the launch list with two queries per lane and may freeze (sf_icp_set_wide_scan_points;
        default 131 072).  Call before set_source*."""
        _check(self.lib.sf_icp_set_wide_scan_points(self.h, C.c_int64(int(points))))

    def set_pipeline(self, on=True):
        """Overlap of consecutive align_batch_async calls on unchanged inputs (sf_icp_set_pipeline, default on)."""
        _check(self.lib.sf_icp_set_pipeline(self.h, C.c_int(int(bool(on)))))

    def set_tile_search(self, on="auto"):
        """Tile search (sf_icp_set_tile_search): the searching launches of large batches served out of LDS tile by tile, see
        include/slamfusion.h.  False / "off", "auto" (default: batches of at least 2 M queries), True / "always"."""
        code = {False: 0, "off": 0, "auto": 1, True: 2, "always": 2}[on]
        _check(self.lib.sf_icp_set_tile_search(self.h, C.c_int(code)))

    def tile_info(self):
        """Of the last alignment (sf_icp_tile_info); the counters are filled while profiling is on."""
        a = (C.c_int64 * 12)()
        _check(self.lib.sf_icp_tile_info(self.h, a))
        return {"on": bool(a[0]), "cells_per_tile": [a[1], a[2], a[3]], "tiles": [a[4], a[5], a[6]], "searched": a[7], "from_lds": a[8], "left_region": a[9],
                "beyond_ring_1": a[10], "tiles_too_dense": a[11]}

    def set_freeze_params(self, guard_scale=8.0, guard_min=2.0e-5, guard_max=3.0e-4, max_tries=3, from_launch=5):
        _check(self.lib.sf_icp_set_freeze_params(self.h, C.c_float(guard_scale), C.c_float(guard_min), C.c_float(guard_max), C.c_int(max_tries), C.c_int(from_launch)))

    def freeze_stats(self):
        """Of the last batched alignment, summed over its scans (sf_icp_freeze_stats)."""
        a = (C.c_int64 * 5)()
        _check(self.lib.sf_icp_freeze_stats(self.h, a))
        return {"froze": a[0], "thawed": a[1], "failed": a[2], "active_queries": a[3], "frozen_at_end": a[4]}

    def set_defer_search(self, on=True):
        """Deferred search of the frozen-pairs schedule (sf_icp_set_defer_search, default on): the stragglers of the last verifying
        launch before the first chance to freeze go to a dense pass instead of being searched in place."""
        _check(self.lib.sf_icp_set_defer_search(self.h, C.c_int(int(bool(on)))))

    def set_neighbour_research(self, from_launch=2):
        """sf_icp_set_neighbour_research: the first launch index (>= 1) that consults the map's neighbour table; negative: never."""
        _check(self.lib.sf_icp_set_neighbour_research(self.h, C.c_int(int(from_launch))))

    def neighbour_stats(self):
        """Of the last alignment, profiled runs only (sf_icp_neighbour_stats)."""
        a = (C.c_int64 * 3)()
        _check(self.lib.sf_icp_neighbour_stats(self.h, a))
        return {"served": a[0], "not_served": a[1], "waves_searched": a[2]}

    def neighbour_gap_stats(self):
        """neighbour_stats and "by_gap": the served queries the nearest gap alone settled (sf_icp_neighbour_gap_stats)."""
        a = (C.c_int64 * 4)()
        _check(self.lib.sf_icp_neighbour_gap_stats(self.h, a))
        return {"served": a[0], "not_served": a[1], "waves_searched": a[2], "by_gap": a[3]}

    def defer_stats(self):
        """Of the last batched alignment (sf_icp_defer_stats): queries that went to the dense pass, waves that hit the cap."""
        a = (C.c_int64 * 2)()
        _check(self.lib.sf_icp_defer_stats(self.h, a))
        return {"deferred_queries": a[0], "capped_waves": a[1]}

    def lookup_launch_stats(self):
        """Of the last batched alignment (sf_icp_lookup_launch_stats): how many launches ran in look-up form and the index of the
        first (-1: none), the queries they deferred and their capped waves."""
        a = (C.c_int64 * 4)()
        _check(self.lib.sf_icp_lookup_launch_stats(self.h, a))
        return {"launches": a[0], "deferred_queries": a[1], "capped_waves": a[2], "first": a[3]}

    def set_query_order(self, order="auto"):
        """'auto' | 'as_given' | 'cell' (SF_ORDER_*): the order a scan's points are walked in."""
        _check(self.lib.sf_icp_set_query_order(self.h, C.c_int({"auto": 0, "as_given": 1, "cell": 2}[order])))

    def align(self, mode="ref_cpp"):
        r = IcpResult()
        _check(self.lib.sf_icp_align(self.h, C.c_int(MODES[mode]), C.byref(r)))
        return r.as_dict()

    def align_batch(self, mode="p2plane"):
        arr = (IcpResult * self.batch)()
        _check(self.lib.sf_icp_align_batch(self.h, C.c_int(MODES[mode]), arr))
        self._prev_batch, self._last_batch = getattr(self, "_last_batch", None), self.batch
        return [r.as_dict() for r in arr]

    def align_batch_async(self, mode="p2plane"):
        _check(self.lib.sf_icp_align_batch_async(self.h, C.c_int(MODES[mode])))
        # how many scans the latest / the previous enqueued alignment registered (a source set since belongs to the next one)
        self._prev_batch, self._last_batch = getattr(self, "_last_batch", None), self.batch

    def fetch_results(self, raw=False):
        """Results of the LATEST enqueued alignment, as it was enqueued."""
        arr = (IcpResult * int(getattr(self, "_last_batch", None) or self.batch))()
        _check(self.lib.sf_icp_fetch_results(self.h, arr))
        return arr if raw else [r.as_dict() for r in arr]

    def fetch_previous(self, batch=None, raw=False):
        """Results of the alignment enqueued before the latest one (both asynchronous, no fetch between them): waits for that
        one only; raw: the ctypes array as it came."""
        arr = (IcpResult * int(batch or getattr(self, "_prev_batch", None) or self.batch))()
        _check(self.lib.sf_icp_fetch_previous(self.h, arr))
        return arr if raw else [r.as_dict() for r in arr]

    # multi-GPU stepping
    def set_shard(self, x_lo, x_hi):
        _check(self.lib.sf_icp_set_shard(self.h, C.c_float(x_lo), C.c_float(x_hi)))

    def set_exchange_buffer(self, ptr, nbytes):
        _check(self.lib.sf_icp_set_exchange_buffer(self.h, C.c_void_p(ptr), C.c_int64(nbytes)))

    def exchange_ptr(self):
        n = C.c_int64()
        p = self.lib.sf_icp_exchange_ptr(self.h, C.byref(n))
        return p, n.value

    def set_shard_margin(self, margin_m):
        _check(self.lib.sf_icp_set_shard_margin(self.h, C.c_float(margin_m)))

    def step_begin(self, mode, first):
        _check(self.lib.sf_icp_step_begin(self.h, C.c_int(MODES[mode]), C.c_int(int(first))))
        if int(first) == 1:                                   # a new alignment: fetch_results returns ITS scans (a source set since an earlier align_batch_async may hold another number)
            self._last_batch = self.batch

    def step_end(self, mode, last):
        _check(self.lib.sf_icp_step_end(self.h, C.c_int(MODES[mode]), C.c_int(int(last))))

    def align_sharded(self, mode, comm):
        """The whole sharded alignment from the C side (RCCL all-reduce per iteration on the context's stream)."""
        arr = (IcpResult * self.batch)()
        resumes = C.c_int()
        _check(self.lib.sf_icp_align_sharded(self.h, C.c_int(MODES[mode]), comm.h, arr, C.byref(resumes)))
        self.resumes = resumes.value
        return [r.as_dict() for r in arr]

    def align_sharded_async(self, mode, comm, first=1):
        _check(self.lib.sf_icp_align_sharded_async(self.h, C.c_int(MODES[mode]), comm.h, C.c_int(first)))

    def owned_counts(self):
        out = np.empty(self.batch, np.int64)
        _check(self.lib.sf_icp_owned_counts(self.h, _p(out), C.c_int(self.batch)))
        return out

    def profile_enable(self, on=True):
        _check(self.lib.sf_icp_profile_enable(self.h, C.c_int(int(on))))

    def profile_read(self):
        n, ms = C.c_int64(), C.c_double()
        _check(self.lib.sf_icp_profile_read(self.h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def profile_launches(self):
        """-> (ms[k], searched_queries[k], searched_waves[k]) of every profiled NN launch, in launch order"""
        n = C.c_int64()
        _check(self.lib.sf_icp_profile_read_launches(self.h, None, None, None, C.c_int64(0), C.byref(n)))
        ms = np.empty(max(n.value, 1), np.float32)
        q = np.empty(max(n.value, 1), np.uint32)
        w = np.empty(max(n.value, 1), np.uint32)
        _check(self.lib.sf_icp_profile_read_launches(self.h, _p(ms), _p(q), _p(w), C.c_int64(len(ms)), C.byref(n)))
        return ms[:n.value], q[:n.value], w[:n.value]

    def profile_phases(self, kind):
        """Durations [ms] of one phase of the sharded path while profiling (PROF_REDUCE / COLLECTIVE / SOLVE / SHARD_BUILD)."""
        n = C.c_int64()
        _check(self.lib.sf_icp_profile_read_phases(self.h, C.c_int(kind), None, C.c_int64(0), C.byref(n)))
        ms = np.empty(max(n.value, 1), np.float32)
        _check(self.lib.sf_icp_profile_read_phases(self.h, C.c_int(kind), _p(ms), C.c_int64(len(ms)), C.byref(n)))
        return ms[:n.value]

    def close(self):
        if self.h:
            self.lib.sf_icp_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def global_register(src_cloud, src_features, dst_cloud, dst_features, distance_threshold, ratio=0, edge_similarity=0.9, num_hypotheses=4096, refine_rounds=2,
                    min_inliers=3, top_k=0, seed=0, icp=None, icp_mode="o3d_p2p", profile=False, src_keypoints=None, dst_keypoints=None):
    """Pose of src_cloud in dst_cloud without a prior: the mutual matches of the two descriptor sets, then Cloud.register_pairs on them.
    icp: None, or a factory icp(batch) -> an Icp with its target set; the top_k candidates and the refit pose are then refined as ONE
    batch of the batched ICP and the result with the best (fitness, -rmse) is returned.
    src_keypoints / dst_keypoints: None, or an int array of indices into that side's cloud (Cloud.iss_keypoints, Map.iss_keypoints);
    only those rows of its descriptor set are matched (Features.gather) and the matcher's pairs are mapped back to cloud indices.
    -> dict(T float64 [4, 4], found, fitness, rmse, pairs (cloud indices), match_stats, ransac: the register_pairs dict, icp: the batch
    results or None, chosen: the index into the batch, the refit pose last, or None)."""
    src_rows = None if src_keypoints is None else _rows(src_keypoints)
    dst_rows = None if dst_keypoints is None else _rows(dst_keypoints)
    src_set = src_features if src_rows is None else src_features.gather(src_rows)
    dst_set = dst_features if dst_rows is None else dst_features.gather(dst_rows)
    match = src_set.match(dst_set, ratio=ratio, mutual=True, profile=profile)
    pairs = match["pairs"]
    if src_rows is not None or dst_rows is not None:
        pairs = pairs.copy()
        if src_rows is not None:
            pairs[:, 0] = src_rows[pairs[:, 0]]
        if dst_rows is not None:
            pairs[:, 1] = dst_rows[pairs[:, 1]]
    reg = src_cloud.register_pairs(dst_cloud, pairs, distance_threshold, edge_similarity, num_hypotheses, refine_rounds, min_inliers, top_k, seed, profile)
    out = dict(T=reg["T"], found=reg["found"], fitness=reg["stats"]["fitness"], rmse=reg["stats"]["rmse"], pairs=pairs, match_stats=match["stats"], ransac=reg,
               icp=None, chosen=None)
    if icp is None or not reg["found"]:
        return out
    inits = [c["T"] for c in reg["top"]] + [reg["T"]]
    scan = src_cloud.download()
    solver = icp(len(inits))
    solver.set_source_batch(np.broadcast_to(scan, (len(inits),) + scan.shape))
    solver.set_initial_batch(np.stack(inits))
    res = solver.align_batch(icp_mode)
    chosen = max(range(len(res)), key=lambda k: (res[k]["fitness"], -res[k]["rmse"], k))
    out.update(T=res[chosen]["T64"], fitness=res[chosen]["fitness"], rmse=res[chosen]["rmse"], icp=res, chosen=chosen)
    return out


def place_register(db, cloud, k=4, pose=None, icp=None, icp_mode="o3d_p2p"):
    """Pose of `cloud` (a scan in the sensor frame, or seen from `pose`) in the map a PlaceDB's keyframes were taken in, without a
    prior: PlaceDB.query_cloud, then the best candidate T_entry . Rz(shift 2 pi / num_sectors).
    icp: None, or a factory icp(batch) -> an Icp with its target set; the candidate poses are then refined as ONE batch of the batched
    ICP and the result with the best (fitness, -rmse) is returned.
    -> dict(T float64 [4, 4], found, index, shift, dist (of the candidate T came from), candidates: the query_cloud dict, icp: the
    batch results or None, chosen: the index into the candidates)."""
    cand = db.query_cloud(cloud, k, pose)
    live = [j for j in range(cand["idx"].shape[1]) if cand["idx"][0, j] >= 0]
    out = dict(T=np.eye(4), found=bool(live), index=-1, shift=0, dist=float("inf"), candidates=cand, icp=None, chosen=None)
    if not live:
        return out
    chosen, res = 0, None
    if icp is not None:
        scan = cloud.download()
        if pose is not None:                     # the batch wants the scan in the sensor frame: R^T (p - t)
            T = _f64(pose).reshape(4, 4)
            scan = ((scan.astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
        solver = icp(len(live))
        solver.set_source_batch(np.broadcast_to(scan, (len(live),) + scan.shape))
        solver.set_initial_batch(np.stack([cand["poses"][0, j] for j in live]))
        res = solver.align_batch(icp_mode)
        chosen = max(range(len(res)), key=lambda j: (res[j]["fitness"], -res[j]["rmse"], -j))
    j = live[chosen]
    out.update(T=res[chosen]["T64"] if res is not None else cand["poses"][0, j].copy(), index=int(cand["idx"][0, j]), shift=int(cand["shift"][0, j]),
               dist=float(cand["dist"][0, j]), icp=res, chosen=chosen)
    return out


def align_group(members, mode):
    """Several slabs of one map held by this process on one device (sf_icp_align_group) -> (results, resumes)."""
    n = len(members)
    arr = (IcpResult * members[0].batch)()
    hs = (C.c_void_p * n)(*[m.h for m in members])
    resumes = C.c_int()
    _check(load_library().sf_icp_align_group(hs, C.c_int(n), C.c_int(MODES[mode]), arr, C.byref(resumes)))
    return [r.as_dict() for r in arr], resumes.value


def shard_route(scans, inits, edges, margin):
    """Slab range [lo, hi] of every scan (sf_shard_route)."""
    scans = _f32(scans)
    assert scans.ndim == 3 and scans.shape[2] == 3
    B = scans.shape[0]
    T = None if inits is None else _f64(inits).reshape(B, 16)
    e = _f64(edges)
    lo, hi = np.empty(B, np.int32), np.empty(B, np.int32)
    _check(load_library().sf_shard_route(_p(scans), C.c_int64(scans.shape[1]), C.c_int(B), _p(T) if T is not None else None, _p(e), C.c_int(len(e) - 1),
                                         C.c_double(margin), _p(lo), _p(hi)))
    return lo, hi


def rccl_library_path():
    """The RCCL the process must share: the one inside the torch wheel when torch is importable (its HIP runtime is
    the one this process uses, see load_library), else the system's."""
    try:
        import torch
        p = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
        if os.path.exists(p):
            return p
    except ImportError:
        pass
    return None


class Comm:
    """sf_comm: the communicator the C side all-reduces the normal-equation records on, bound to a context's stream.

    Comm(ctx, nranks, rank, unique_id)        RCCL, created from a 128-byte unique id
    Comm.p2p(ctx, nranks, rank, max_count)    the hand-written P2P transport (hipIpc store-and-flag, fixed rank-order sum):
                                              then .handle() -> bytes, .connect([handles in rank order]) -- or
                                              .rendezvous(name) for ranks of one node without a launcher
    """

    @staticmethod
    def unique_id():
        lib = load_library()
        path = rccl_library_path()
        _check(lib.sf_comm_load_rccl(path.encode() if path else None))
        buf = (C.c_char * 128)()
        _check(lib.sf_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, ctx, nranks, rank, unique_id=None, _p2p_max_count=None):
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p()
        if _p2p_max_count is not None:
            _check(self.lib.sf_comm_p2p_create(ctx.h, C.c_int(nranks), C.c_int(rank), C.c_int64(int(_p2p_max_count)), C.byref(self.h)))
            self.kind = "p2p"
        else:
            path = rccl_library_path()
            _check(self.lib.sf_comm_load_rccl(path.encode() if path else None))
            assert len(unique_id) == 128
            _check(self.lib.sf_comm_create(ctx.h, C.c_int(nranks), C.c_int(rank), (C.c_char * 128).from_buffer_copy(unique_id), C.byref(self.h)))
            self.kind = "rccl"
        self.nranks, self.rank = nranks, rank
        _live.add(self)

    @classmethod
    def p2p(cls, ctx, nranks, rank, max_count):
        return cls(ctx, nranks, rank, _p2p_max_count=max_count)

    def handle(self):
        buf = (C.c_char * 128)()
        _check(self.lib.sf_comm_p2p_handle(self.h, buf))
        return bytes(buf)

    def connect(self, handles):
        blob = b"".join(handles)
        assert len(blob) == 128 * self.nranks
        _check(self.lib.sf_comm_p2p_connect(self.h, (C.c_char * len(blob)).from_buffer_copy(blob)))

    def rendezvous(self, name, timeout_s=60.0):
        _check(self.lib.sf_comm_p2p_rendezvous(self.h, name.encode(), C.c_double(timeout_s)))

    def set_timeout(self, seconds):
        _check(self.lib.sf_comm_set_timeout(self.h, C.c_double(seconds)))

    def abort(self):
        _check(self.lib.sf_comm_abort(self.h))

    def status(self):
        """Raises SlamFusionError (SF_ERR_COMM) once a collective of this communicator timed out or was aborted."""
        _check(self.lib.sf_comm_status(self.h))

    def allreduce_f64(self, ptr, count):
        _check(self.lib.sf_comm_allreduce_f64(self.h, C.c_void_p(ptr), C.c_int64(count)))

    def close(self):
        if self.h:
            self.lib.sf_comm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BruteForceAlignment:
    """sf_bf: mirrors BruteForceAlignment (brute_force_alignment.h:22-112) setter for setter."""

    def __init__(self, ctx):
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p()
        self._map = None
        _check(self.lib.sf_bf_create(ctx.h, C.byref(self.h)))
        _live.add(self)

    def setXYZStep(self, x, y, z):
        _check(self.lib.sf_bf_set_xyz_step(self.h, C.c_float(x), C.c_float(y), C.c_float(z)))

    def setXYZRange(self, x, y, z):
        _check(self.lib.sf_bf_set_xyz_range(self.h, C.c_float(x), C.c_float(y), C.c_float(z)))

    def setRotationStep(self, v):
        _check(self.lib.sf_bf_set_rotation_step(self.h, C.c_float(v)))

    def setRotationRange(self, v):
        _check(self.lib.sf_bf_set_rotation_range(self.h, C.c_float(v)))

    def setMeanErrorThreshold(self, v):
        _check(self.lib.sf_bf_set_mean_error_threshold(self.h, C.c_float(v)))

    def setInitialGuess(self, T):
        T = _f32(T).reshape(16)
        _check(self.lib.sf_bf_set_initial_guess(self.h, _p(T)))

    def setSourceCloud(self, cloud):
        if isinstance(cloud, Cloud):
            _check(self.lib.sf_bf_set_source_cloud(self.h, cloud.h))
        else:
            xyz = _f32(cloud).reshape(-1, 3)
            _check(self.lib.sf_bf_set_source(self.h, _p(xyz), C.c_int64(len(xyz))))

    def setTargetCloud(self, target):
        if isinstance(target, Map):
            self._map = target
            _check(self.lib.sf_bf_set_target_map(self.h, target.h))
        else:
            xyz = _f32(target).reshape(-1, 3)
            _check(self.lib.sf_bf_set_target(self.h, _p(xyz), C.c_int64(len(xyz))))

    def resetFirstAlignment(self, value):
        _check(self.lib.sf_bf_reset_first_alignment(self.h, C.c_int(int(value))))

    def alignClouds(self):
        found = C.c_int()
        _check(self.lib.sf_bf_align_clouds(self.h, C.byref(found)))
        return bool(found.value)

    def firstAlignmentCompleted(self):
        return bool(self.lib.sf_bf_first_alignment_completed(self.h))

    def getBestTransformation(self):
        T = np.empty(16, np.float32)
        _check(self.lib.sf_bf_get_best_transformation(self.h, _p(T)))
        return T.reshape(4, 4)

    def last_result(self):
        idx, score, ncand = C.c_int32(), C.c_float(), C.c_int32()
        _check(self.lib.sf_bf_last_result(self.h, C.byref(idx), C.byref(score), C.byref(ncand), None, C.c_int64(0)))
        scores = np.empty(max(ncand.value, 1), np.float32)
        _check(self.lib.sf_bf_last_result(self.h, None, None, None, _p(scores), C.c_int64(len(scores))))
        return dict(index=idx.value, score=score.value, n_candidates=ncand.value, scores=scores[:ncand.value])

    def close(self):
        if self.h:
            self.lib.sf_bf_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NodeParams(C.Structure):
    """sf_node_params"""
    _fields_ = [("ref_frame_distance", C.c_float), ("cloud_crop_radius", C.c_float), ("index_cell", C.c_float), ("pcl_crop_order", C.c_int32),
                ("icp_mode", C.c_int32), ("map_is_downsampled", C.c_int32)]


class GpsFix(C.Structure):
    """sf_gps_fix"""
    _fields_ = [("latitude", C.c_double), ("longitude", C.c_double), ("altitude", C.c_double), ("position_covariance", C.c_double * 9)]


class Odom(C.Structure):
    """sf_odom"""
    _fields_ = [("q_wxyz", C.c_double * 4), ("t", C.c_double * 3), ("covariance", C.c_double * 36)]


class NodeOutput(C.Structure):
    """sf_node_output"""
    _fields_ = [("status", C.c_int32), ("recropped", C.c_int32), ("coarse_ran", C.c_int32), ("pad_", C.c_int32), ("n_scan", C.c_int64),
                ("map_T_sensor", C.c_float * 16), ("prior", C.c_float * 16), ("odom_pose", C.c_float * 16), ("gps_pose", C.c_float * 16),
                ("odometry_gain", C.c_float), ("gps_compass_gain", C.c_float), ("icp", IcpResult), ("coarse_icp", IcpResult)]


SF_NODE_OK, SF_NODE_GATED_ALTITUDE, SF_NODE_FIRST_MESSAGE, SF_NODE_COARSE_FAILED = 0, 1, 2, 3
SF_NODE_POSE_MAP_T_SENSOR, SF_NODE_POSE_MAP_T_REF, SF_NODE_POSE_ODOM_PREVIOUS = 0, 1, 2


class _BorrowedIcp(Icp):
    """The icp_ of a Node: same methods, the handle belongs to the node."""

    def __init__(self, ctx, handle):
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p(handle)
        self._map = None
        self.batch = 1

    def close(self):
        self.h = C.c_void_p()


class _BorrowedBf(BruteForceAlignment):
    """The brute_force_alignment_ of a Node."""

    def __init__(self, ctx, handle):
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p(handle)
        self._map = None

    def close(self):
        self.h = C.c_void_p()


class Node:
    """sf_node: LocalizationNode's per-scan callback (localization_node.cpp:263-344) as one library call."""

    def __init__(self, ctx, map_points, map_T_global, altitude_table=None, **params):
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p()
        prm = NodeParams()
        self.lib.sf_node_default_params(C.byref(prm))
        for k, v in params.items():
            if k == "icp_mode":
                v = MODES[v] if isinstance(v, str) else v
            setattr(prm, k, type(getattr(prm, k))(v))
        self.params = prm
        xyz = _f32(map_points).reshape(-1, 3)
        M = _f64(map_T_global).reshape(16)
        tab = _f64(np.zeros((0, 3)) if altitude_table is None else altitude_table).reshape(-1, 3)
        _check(self.lib.sf_node_create(ctx.h, _p(xyz), C.c_int64(len(xyz)), _p(M), _p(tab), C.c_int(len(tab)), C.byref(prm), C.byref(self.h)))
        self.icp = _BorrowedIcp(ctx, self.lib.sf_node_icp(self.h))
        self.bf = _BorrowedBf(ctx, self.lib.sf_node_bf(self.h))
        self._gps, self._odom, self._out = GpsFix(), Odom(), NodeOutput()
        _live.add(self)

    def compass(self, compass_deg):
        _check(self.lib.sf_node_compass(self.h, C.c_double(compass_deg)))

    def _messages(self, gps, odom):
        g, o = self._gps, self._odom
        g.latitude, g.longitude, g.altitude = gps["latitude"], gps["longitude"], gps["altitude"]
        for dst, src, n in ((g.position_covariance, gps["position_covariance"], 9), (o.q_wxyz, odom["q_wxyz"], 4), (o.t, odom["t"], 3), (o.covariance, odom["covariance"], 36)):
            a = np.ascontiguousarray(src, dtype=np.float64)           # one block copy instead of a Python-level loop over the elements
            if a.size != n:
                raise SlamFusionError("message field has %d values, %d expected" % (a.size, n))
            C.memmove(dst, a.ctypes.data, 8 * n)
        return g, o

    def callback(self, scan, gps, odom):
        """scan: float32 [n, 3] or a PointCloud2-like message (data, width, height, point_step, row_step, offsets);
        returns the sf_node_output structure (valid until the next call)."""
        g, o = self._messages(gps, odom)
        if hasattr(scan, "point_step"):
            buf, width, height, point_step, row_step, offs, dtype, big = _pc2_layout(scan)
            _check(self.lib.sf_node_callback_pointcloud2(self.h, _p(buf), C.c_int64(buf.size), C.c_int64(width), C.c_int64(height), C.c_int(point_step), C.c_int64(row_step),
                                                         C.c_int(offs[0]), C.c_int(offs[1]), C.c_int(offs[2]), C.c_int(dtype), C.c_int(big), C.byref(g), C.byref(o), C.byref(self._out)))
        else:
            xyz = _f32(scan).reshape(-1, 3)
            _check(self.lib.sf_node_callback_xyz(self.h, _p(xyz), C.c_int64(len(xyz)), C.byref(g), C.byref(o), C.byref(self._out)))
        return self._out

    def get_pose(self, which=SF_NODE_POSE_MAP_T_SENSOR):
        T = np.empty(16, np.float32)
        _check(self.lib.sf_node_get_pose(self.h, C.c_int(which), _p(T)))
        return T.reshape(4, 4)

    def set_pose(self, which, T):
        T = _f32(T).reshape(16)
        _check(self.lib.sf_node_set_pose(self.h, C.c_int(which), _p(T)))

    def coarse_alignment_complete(self):
        return bool(self.lib.sf_node_coarse_alignment_complete(self.h))

    def set_coarse_alignment_complete(self, v=True):
        _check(self.lib.sf_node_set_coarse_alignment_complete(self.h, C.c_int(int(v))))

    def close(self):
        if self.h:
            self.icp.close()
            self.bf.close()
            self.lib.sf_node_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pcd_read(path):
    lib = load_library()
    ptr, n = C.POINTER(C.c_float)(), C.c_int64()
    _check(lib.sf_pcd_read(str(path).encode(), C.byref(ptr), C.byref(n)))
    out = np.ctypeslib.as_array(ptr, shape=(max(n.value, 1) * 3,))[:n.value * 3].reshape(-1, 3).copy()
    lib.sf_free(ptr)
    return out


def pcd_write_binary(path, xyz):
    xyz = _f32(xyz).reshape(-1, 3)
    _check(load_library().sf_pcd_write_binary(str(path).encode(), _p(xyz), C.c_int64(len(xyz))))


class MapDataSaver:
    """sf_recorder: the file writers of mapping/src/map_data_save_node.cpp (tiles + the two text logs)."""

    def __init__(self, map_data_path):
        self.lib = load_library()
        self.lib.sf_recorder_compass_yaw.restype = C.c_double
        self.h = C.c_void_p()
        _check(self.lib.sf_recorder_create(str(map_data_path).encode(), C.byref(self.h)))
        self.current_compass_yaw = 0.0

    def compassCallback(self, hdg_deg):
        self.current_compass_yaw = float(self.lib.sf_recorder_compass_yaw(C.c_double(hdg_deg)))

    def mappingCallback(self, xyz, odom_xyz, lat, lon, alt):
        xyz, o = _f32(xyz).reshape(-1, 3), _f64(odom_xyz).reshape(3)
        _check(self.lib.sf_recorder_add(self.h, _p(xyz), C.c_int64(len(xyz)), _p(o), C.c_double(lat), C.c_double(lon), C.c_double(alt),
                                        C.c_double(self.current_compass_yaw)))

    def onShutdown(self):
        _check(self.lib.sf_recorder_shutdown(self.h))

    def __del__(self):
        try:
            if self.h:
                self.lib.sf_recorder_destroy(self.h)
                self.h = None
        except Exception:
            pass


class GlobalMapFramesManager:
    """sf_frames: GlobalMapFramesManager of localization/src/global_map_frames_manager.cpp."""

    def __init__(self, data_folder, map_name="map", num_poses_max=50):
        self.lib = load_library()
        self.lib.sf_frames_create.restype = C.c_void_p
        self.lib.sf_frames_get_closest_altitude.restype = C.c_float
        self.h = C.c_void_p(self.lib.sf_frames_create(str(data_folder).encode(), str(map_name).encode(), C.c_int64(num_poses_max)))

    def getMapCloud(self, ctx, voxel_size=0.1):
        cloud = Cloud(ctx)
        cached = C.c_int()
        _check(self.lib.sf_frames_get_map_cloud(self.h, cloud.h, C.c_float(voxel_size), C.byref(cached)))
        self.loaded_cached = bool(cached.value)
        return cloud

    def getMapTGlobal(self):
        T = np.empty(16, np.float64)
        _check(self.lib.sf_frames_get_map_T_global(self.h, _p(T)))
        return T.reshape(4, 4)

    def getClosestAltitude(self, lat, lon):
        return float(self.lib.sf_frames_get_closest_altitude(self.h, C.c_double(lat), C.c_double(lon)))

    def altitude_table(self):
        rows = C.c_int64()
        _check(self.lib.sf_frames_altitude_table(self.h, None, C.c_int64(0), C.byref(rows)))
        tab = np.empty((max(rows.value, 1), 3), np.float64)
        _check(self.lib.sf_frames_altitude_table(self.h, _p(tab), C.c_int64(len(tab)), C.byref(rows)))
        return tab[:rows.value]

    def __del__(self):
        try:
            if self.h:
                self.lib.sf_frames_destroy(self.h)
                self.h = None
        except Exception:
            pass


# ------------------------------------------------------------------ pose fusion (host C++)
def quat_to_pose(q_wxyz, t):
    q, t = _f64(q_wxyz), _f64(t)
    T = np.empty(16, np.float32)
    load_library().sf_fusion_quat_to_pose(_p(q), _p(t), _p(T))
    return T.reshape(4, 4)


def odom_prediction(map_T_sensor, odom_T_prev, odom_T_cur):
    a, b, c = (_f32(x).reshape(16) for x in (map_T_sensor, odom_T_prev, odom_T_cur))
    out = np.empty(16, np.float32)
    load_library().sf_fusion_odom_prediction(_p(a), _p(b), _p(c), _p(out))
    return out.reshape(4, 4)


def compass_to_yaw(deg):
    return float(load_library().sf_fusion_compass_to_yaw(C.c_double(deg)))


def ll_to_utm(lat, lon):
    n, e = C.c_double(), C.c_double()
    load_library().sf_fusion_ll_to_utm(C.c_double(lat), C.c_double(lon), C.byref(n), C.byref(e))
    return n.value, e.value


def closest_altitude(table, lat, lon):
    table = _f64(table).reshape(-1, 3)
    return float(load_library().sf_fusion_closest_altitude(_p(table), C.c_int(len(table)), C.c_double(lat), C.c_double(lon)))


def gps_pose(map_T_global, yaw, lat, lon, table_alt):
    M = _f64(map_T_global).reshape(16)
    out = np.empty(16, np.float32)
    load_library().sf_fusion_gps_pose(_p(M), C.c_float(yaw), C.c_double(lat), C.c_double(lon), C.c_float(table_alt), _p(out))
    return out.reshape(4, 4)


def pose_gains(gps_cov, odom_cov, fixed=False):
    g, o = _f64(gps_cov).reshape(9), _f64(odom_cov).reshape(36)
    a, b = C.c_float(), C.c_float()
    load_library().sf_fusion_pose_gains(_p(g), _p(o), C.c_int(int(fixed)), C.byref(a), C.byref(b))
    return a.value, b.value


def blend(g_odom, T_odom, g_gps, T_gps):
    a, b = _f32(T_odom).reshape(16), _f32(T_gps).reshape(16)
    out = np.empty(16, np.float32)
    load_library().sf_fusion_blend(C.c_float(g_odom), _p(a), C.c_float(g_gps), _p(b), _p(out))
    return out.reshape(4, 4)


def map_T_global(latlonalt, yaw):
    l, y = _f64(latlonalt).reshape(-1, 3), _f32(yaw)
    out = np.empty(16, np.float64)
    load_library().sf_fusion_map_T_global(_p(l), _p(y), C.c_int(len(l)), _p(out))
    return out.reshape(4, 4)


def mat4f_inverse(A):
    A = _f32(A).reshape(16)
    out = np.empty(16, np.float32)
    load_library().sf_fusion_mat4f_inverse(_p(A), _p(out))
    return out.reshape(4, 4)


def mat4f_mul(A, B):
    A, B = _f32(A).reshape(16), _f32(B).reshape(16)
    out = np.empty(16, np.float32)
    load_library().sf_fusion_mat4f_mul(_p(A), _p(B), _p(out))
    return out.reshape(4, 4)


class Ekf:
    """sf_ekf: error-state EKF pose prior with IMU pre-integration (extension f-4; the reference has none)."""

    def __init__(self):
        self.lib = load_library()
        self.h = C.c_void_p()
        _check(self.lib.sf_ekf_create(C.byref(self.h)))

    def reset(self, T, v=None, P_diag=None):
        T = _f64(T).reshape(16)
        v = None if v is None else _f64(v).reshape(3)
        P = None if P_diag is None else _f64(P_diag).reshape(9)
        _check(self.lib.sf_ekf_reset(self.h, _p(T), _p(v) if v is not None else None, _p(P) if P is not None else None))

    def set_noise(self, gyro_sigma, accel_sigma, gravity=None):
        g = None if gravity is None else _f64(gravity).reshape(3)
        _check(self.lib.sf_ekf_set_noise(self.h, C.c_double(gyro_sigma), C.c_double(accel_sigma), _p(g) if g is not None else None))

    def set_bias(self, gyro_bias=None, accel_bias=None, gyro_bias_var=None, accel_bias_var=None):
        args = [None if a is None else _f64(a).reshape(3) for a in (gyro_bias, accel_bias, gyro_bias_var, accel_bias_var)]
        _check(self.lib.sf_ekf_set_bias(self.h, *[_p(a) if a is not None else None for a in args]))

    def set_bias_noise(self, gyro_bias_walk, accel_bias_walk):
        _check(self.lib.sf_ekf_set_bias_noise(self.h, C.c_double(gyro_bias_walk), C.c_double(accel_bias_walk)))

    def full_state(self):
        """-> (gyro bias, accelerometer bias, 15x15 covariance over dp, dv, dtheta, dbg, dba)"""
        bg, ba, P = np.empty(3), np.empty(3), np.empty(225)
        _check(self.lib.sf_ekf_get_full(self.h, _p(bg), _p(ba), _p(P)))
        return bg, ba, P.reshape(15, 15)

    def predict_imu(self, gyro, accel, dt):
        gyro, accel = _f64(gyro).reshape(-1, 3), _f64(accel).reshape(-1, 3)
        assert len(gyro) == len(accel)
        _check(self.lib.sf_ekf_predict_imu(self.h, _p(gyro), _p(accel), C.c_int64(len(gyro)), C.c_double(dt)))

    def predict_odometry(self, T_prev, T_cur, cov_pos=None, cov_rot=None):
        a, b = _f64(T_prev).reshape(16), _f64(T_cur).reshape(16)
        cp = None if cov_pos is None else _f64(cov_pos).reshape(3)
        cr = None if cov_rot is None else _f64(cov_rot).reshape(3)
        _check(self.lib.sf_ekf_predict_odometry(self.h, _p(a), _p(b), _p(cp) if cp is not None else None, _p(cr) if cr is not None else None))

    def update_position(self, z, cov):
        z, cov = _f64(z).reshape(3), _f64(cov).reshape(9)
        _check(self.lib.sf_ekf_update_position(self.h, _p(z), _p(cov)))

    def update_yaw(self, yaw, var):
        _check(self.lib.sf_ekf_update_yaw(self.h, C.c_double(yaw), C.c_double(var)))

    def update_pose(self, T, cov_pos, cov_rot):
        T, cp, cr = _f64(T).reshape(16), _f64(cov_pos).reshape(3), _f64(cov_rot).reshape(3)
        _check(self.lib.sf_ekf_update_pose(self.h, _p(T), _p(cp), _p(cr)))

    def update_pose_cov(self, T, cov):
        """Pose update with the ICP's 6x6 covariance (Icp.fetch_covariance()[i]["cov"], order (w, t), left perturbation)."""
        T, cov = _f64(T).reshape(16), _f64(cov).reshape(36)
        _check(self.lib.sf_ekf_update_pose_cov(self.h, _p(T), _p(cov)))

    def state(self):
        T, v, P = np.empty(16), np.empty(3), np.empty(81)
        _check(self.lib.sf_ekf_get(self.h, _p(T), _p(v), _p(P)))
        return T.reshape(4, 4), v, P.reshape(9, 9)

    def close(self):
        if self.h:
            self.lib.sf_ekf_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StochasticFilter:
    """sf_sfilter: StochasticFilter of localization/src/stochastic_filter.cpp."""

    def __init__(self, queue_size=10, n_std_dev_threshold=1.0):
        self.lib = load_library()
        self.q = queue_size
        self.h = C.c_void_p(self.lib.sf_sfilter_create(C.c_int(queue_size), C.c_float(n_std_dev_threshold)))
        if not self.h:
            raise SlamFusionError("sf_sfilter_create failed")

    def setMaximumLinearVelocity(self, v):
        self.lib.sf_sfilter_set_maximum_linear_velocity(self.h, C.c_float(v))

    def weights(self):
        w = np.empty(self.q, np.float32)
        self.lib.sf_sfilter_weights(self.h, _p(w))
        return w

    def addPoseToQueue(self, pose):
        p = _f32(pose).reshape(16)
        self.lib.sf_sfilter_add_pose_to_queue(self.h, _p(p))

    def computePoseZScore(self, prev, cur):
        a, b = _f32(prev).reshape(16), _f32(cur).reshape(16)
        return float(self.lib.sf_sfilter_pose_zscore(self.h, _p(a), _p(b)))

    def applyGaussianFilterToCurrentPose(self, prev, cur):
        a, b = _f32(prev).reshape(16), _f32(cur).reshape(16)
        out = np.empty(16, np.float32)
        self.lib.sf_sfilter_apply_gaussian_filter(self.h, _p(a), _p(b), _p(out))
        return out.reshape(4, 4)

    def __del__(self):
        try:
            if self.h:
                self.lib.sf_sfilter_destroy(self.h)
                self.h = None
        except Exception:
            pass
