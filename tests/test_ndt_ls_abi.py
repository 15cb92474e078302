"""The ABI surface of the NDT line search and levels (include/slamfusion.h: sf_ndt_line_search, sf_ndt_ls_row, sf_ndt_set_line_search,
sf_ndt_scores, sf_ndt_line_search_read, sf_ndt_align_levels): declared in the header in their place, exported by the library, mirrored
by api.NdtLineSearch / NdtLsRow and wrapped by api.Ndt / api.NdtPyramid.  No device call."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARATIONS = (
    r"#define SF_NDT_FLAG_LINE_SEARCH_STALLED 2",
    r"#define SF_NDT_MAX_TRIALS 16",
    r"typedef struct { int32_t trials, pad; double step_max, armijo; } sf_ndt_line_search;",
    r"typedef struct { double alpha_max, raw_length, phi0, slope, delta[6], phi[16]; int64_t n_terms[16]; int32_t chosen, trials; } sf_ndt_ls_row;",
    r"void sf_ndt_default_line_search(sf_ndt_line_search *p);",
    r"int sf_ndt_set_line_search(sf_ndt *ndt, const sf_ndt_line_search *p);",
    r"int sf_ndt_scores(sf_ndt *ndt, const double *poses, int64_t k, double *score, int64_t *n_terms);",
    r"int sf_ndt_line_search_read(sf_ndt *ndt, sf_ndt_ls_row *rows, int64_t cap, int64_t *n);",
    r"int sf_ndt_align_levels(sf_ndt *const *levels, int n_levels, const double *inits, sf_ndt_result *out , sf_ndt_result *per_level );",
)
SYMBOLS = ("sf_ndt_default_line_search", "sf_ndt_set_line_search", "sf_ndt_scores", "sf_ndt_line_search_read", "sf_ndt_align_levels")


def _header():
    with open(os.path.join(ROOT, "include", "slamfusion.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"\s+", " ", text)


def test_header_declares_the_calls_in_their_place():
    text = _header()
    for decl in DECLARATIONS:
        assert re.sub(r"\s+", " ", decl) in text, decl
    # behind the NDT block, before the measurement switch, in the order of the issue
    at = [text.index(s) for s in ("int sf_ndt_stats_read(", "#define SF_NDT_FLAG_LINE_SEARCH_STALLED", "#define SF_NDT_MAX_TRIALS", "} sf_ndt_line_search;", "} sf_ndt_ls_row;",
                                  "void sf_ndt_default_line_search(", "int sf_ndt_set_line_search(", "int sf_ndt_scores(", "int sf_ndt_line_search_read(",
                                  "int sf_ndt_align_levels(", "int sf_map_profile_launches(")]
    assert at == sorted(at)
    with open(os.path.join(ROOT, "include", "slamfusion.h")) as f:
        raw = f.read()
    rule = raw[raw.index("Backtracking line search"):raw.index("#define SF_NDT_FLAG_LINE_SEARCH_STALLED")]   # the rule is stated in the header
    for words in ("alpha_max = raw > step_max ? step_max / raw : 1.0", "((((g0 d0 + g1 d1) + g2 d2) + g3 d3) + g4 d4) + g5 d5", "ldexp(alpha_max, -k)",
                  "phi_k <= phi0 + (armijo * alpha_k) * slope", "SF_NDT_FLAG_LINE_SEARCH_STALLED", "alpha_k * raw < transformation_epsilon"):
        assert words in rule, words


def test_library_exports_the_calls(api):
    lib = api.load_library()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None, name


def test_structs_and_defaults(api):
    names = ["trials", "pad", "step_max", "armijo"]
    assert ctypes.sizeof(api.NdtLineSearch) == 24 and [f[0] for f in api.NdtLineSearch._fields_] == names
    assert [getattr(api.NdtLineSearch, n).offset for n in names] == [0, 4, 8, 16]
    names = ["alpha_max", "raw_length", "phi0", "slope", "delta", "phi", "n_terms", "chosen", "trials"]
    assert ctypes.sizeof(api.NdtLsRow) == 344 and [f[0] for f in api.NdtLsRow._fields_] == names
    assert [getattr(api.NdtLsRow, n).offset for n in names] == [0, 8, 16, 24, 32, 80, 208, 336, 340]
    p = api.NdtLineSearch(9, 9, 9.0, 9.0)
    api.load_library().sf_ndt_default_line_search(ctypes.byref(p))
    assert p.as_dict() == dict(trials=8, step_max=1.0, armijo=1e-4) and p.pad == 0
    assert (api.SF_NDT_FLAG_NO_OVERLAP, api.SF_NDT_FLAG_LINE_SEARCH_STALLED, api.SF_NDT_MAX_TRIALS) == (1, 2, 16)
    r = api.NdtLsRow()
    r.alpha_max, r.raw_length, r.phi0, r.slope, r.delta[5], r.phi[2], r.n_terms[2], r.chosen, r.trials = 0.5, 2.0, -3.0, -4.0, 5.0, 6.0, 7, 2, 3
    d = r.as_dict()
    assert d["alpha_max"] == 0.5 and d["raw_length"] == 2.0 and d["phi0"] == -3.0 and d["slope"] == -4.0 and d["delta"].shape == (6,) and d["delta"][5] == 5.0
    assert d["phi"].shape == (3,) and d["phi"][2] == 6.0 and d["n_terms"].shape == (3,) and d["n_terms"][2] == 7 and d["chosen"] == 2 and d["trials"] == 3


def test_wrapper_signatures(api):
    p = inspect.signature(api.Ndt.set_line_search).parameters
    assert list(p) == ["self", "trials", "step_max", "armijo"] and [v.default for v in p.values()][1:] == [8, 1.0, 1e-4]
    assert list(inspect.signature(api.Ndt.scores).parameters) == ["self", "source", "poses"]
    assert list(inspect.signature(api.Ndt.line_search_rows).parameters) == ["self"]
    p = inspect.signature(api.NdtPyramid.__init__).parameters
    assert list(p) == ["self", "ctx", "target", "resolutions", "line_search", "ndt_kwargs"] and p["line_search"].default is True
    assert p["ndt_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    p = inspect.signature(api.NdtPyramid.align).parameters
    assert list(p) == ["self", "source", "init"] and p["init"].default is None
    assert list(inspect.signature(api.NdtPyramid.align_batch).parameters) == ["self", "sources", "inits"]
    assert list(inspect.signature(api.NdtPyramid.close).parameters) == ["self"]


def _refused(lib, call, *args):
    assert call(*args) == -1                                   # SF_ERR_INVALID
    assert b"bad arguments" in lib.sf_last_error()


def test_argument_checks_without_a_device(api):
    """What the library refuses before it touches a device.  The checks of the line-search parameters come before the object is
    looked at: a block of zeroed host memory stands in for it here and is never read or written (every call below is refused)."""
    lib = api.load_library()
    good = api.NdtLineSearch()
    lib.sf_ndt_default_line_search(ctypes.byref(good))
    res, row, n = api.NdtResult(), api.NdtLsRow(), ctypes.c_int64(-7)
    pose = (ctypes.c_double * 16)()
    score, terms = ctypes.c_double(-7.0), ctypes.c_int64(-7)
    for null_handle in (lambda: lib.sf_ndt_set_line_search(None, ctypes.byref(good)), lambda: lib.sf_ndt_set_line_search(None, None),
                        lambda: lib.sf_ndt_scores(None, pose, ctypes.c_int64(1), ctypes.byref(score), ctypes.byref(terms)),
                        lambda: lib.sf_ndt_line_search_read(None, ctypes.byref(row), ctypes.c_int64(1), ctypes.byref(n)),
                        lambda: lib.sf_ndt_align_levels(None, 1, pose, ctypes.byref(res), None)):
        _refused(lib, null_handle)
    assert n.value == -7 and score.value == -7.0 and terms.value == -7
    stand_in = ctypes.create_string_buffer(1 << 16)
    bad = dict(trials=(-1, 17, 1 << 20), step_max=(0.0, -1.0, float("inf"), float("nan")), armijo=(0.0, 1.0, -0.1, 1.5, float("nan")))
    for field, values in bad.items():
        for v in values:
            p = api.NdtLineSearch()
            lib.sf_ndt_default_line_search(ctypes.byref(p))
            setattr(p, field, v)
            _refused(lib, lib.sf_ndt_set_line_search, stand_in, ctypes.byref(p))
    assert stand_in.raw == bytes(1 << 16)
    levels = (ctypes.c_void_p * 2)(ctypes.addressof(stand_in), None)
    for n_levels in (0, -3):
        _refused(lib, lib.sf_ndt_align_levels, levels, n_levels, pose, ctypes.byref(res), None)
    _refused(lib, lib.sf_ndt_align_levels, levels, 1, None, ctypes.byref(res), None)
    _refused(lib, lib.sf_ndt_align_levels, levels, 1, pose, None, None)
    _refused(lib, lib.sf_ndt_align_levels, levels, 1, pose, ctypes.byref(res), None)       # a level without target or source (the zeroed stand-in)
    levels = (ctypes.c_void_p * 2)(None, None)
    _refused(lib, lib.sf_ndt_align_levels, levels, 2, pose, ctypes.byref(res), None)       # a NULL level
    lib.sf_ndt_default_line_search(None)                       # a no-op


def test_the_version_stays(api):
    assert api.load_library().sf_version() == 210
