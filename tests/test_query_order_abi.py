"""The hook of the query ordering (sf_test_query_order): declared at the end of the hook block of include/slamfusion.h, exported by
the library, wrapped by api.hook_query_order, and refusing bad arguments before any device call.  And the rule of the plain
path on the host side: run_order_sort hands uniform, one-digit sorts to k_order_move through launch_order_plain and reserves the
id array only for the forms that need ids between their passes.  tests/test_gpu_query_order.py runs the kernels."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam_sensor_fusion_amd", "csrc")
DECLARATION = (r"int sf_test_query_order(sf_map *map, const float *points, int batch, int64_t n, const double *poses, int form, int table, "
               r"uint16_t *keys, float *ordered);")


def test_header_declares_the_hook_at_the_end_of_the_hook_block():
    with open(os.path.join(ROOT, "include", "slamfusion.h")) as f:
        text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))
    assert DECLARATION in text
    assert text.index("int sf_test_cloud_minmax(") < text.index("int sf_test_query_order(")


def test_library_exports_and_wraps_it(api):
    lib = api.load_library()
    assert lib.sf_test_query_order is not None
    assert list(inspect.signature(api.hook_query_order).parameters) == ["map_", "points", "poses", "form", "table"]
    assert lib.sf_test_query_order(None, None, 1, 1, None, 1, 0, None, None) != 0          # refused before any device call
    assert "sf_test_query_order" in lib.sf_last_error().decode()


def test_the_plain_path_takes_the_move_kernel_and_no_ids():
    with open(os.path.join(CSRC, "sf_icp_order_host.hpp")) as f:
        text = f.read()
    body = text[text.index("int run_order_sort("):text.index("int order_queries(")]
    plain = body[body.index("if (!icp->tile_on && !seg_off && !src_idx)"):]
    plain = plain[:plain.index("return SF_OK;")]
    assert "launch_order_plain(s, src, kf, keys, counts, 1, nullptr, nullptr, xq)" in plain
    assert body.index("return SF_OK;") < body.index("ln.qidx.reserve(")                     # the ids are reserved behind the plain path's return
    helper = text[text.index("void launch_order_plain("):text.index("int run_order_sort(")]
    assert helper.index("k_order_hist") < helper.index("k_order_scan") < helper.index("k_order_move") < helper.index("k_order_scatter") < helper.index("k_order_gather,")
