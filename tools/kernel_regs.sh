#!/bin/bash
# VGPRs / occupancy of the search kernels of sf_icp.hip as the compiler reports them:  tools/kernel_regs.sh [extra hipcc flags]
# SF_REGS_SRC=sf_map.hip tools/kernel_regs.sh: the normals, patch, k-NN, outlier and clustering kernels of the map index instead
cd "$(dirname "$0")/../slam_sensor_fusion_amd/csrc"
SRC="${SF_REGS_SRC:-sf_icp.hip}"
WIDTH=34; [ -n "$SF_REGS_SRC" ] && WIDTH=40   # (the default report stays as it was)
# SF_REGS_SRC=sf_register.hip tools/kernel_regs.sh: the pose-from-matches kernels (k_reg_*)
# SF_REGS_SRC=sf_keypoint.hip tools/kernel_regs.sh: the ISS keypoint kernels (k_iss_*) and k_features_gather
# SF_REGS_SRC=sf_ndt.hip tools/kernel_regs.sh: the NDT kernels (k_ndt_*), a translation unit of their own: in no other report
# SF_REGS_SRC=sf_visibility.hip tools/kernel_regs.sh: the range-image and visibility kernels (k_ri_*, k_vis_*), a translation unit of their own
# SF_REGS_SRC=sf_place.hip tools/kernel_regs.sh: the Scan Context descriptor, match and selection kernels (k_sc_*), a translation unit of their own
# SF_REGS_SRC=sf_icp.hip tools/kernel_regs.sh: the default report with the query-ordering kernels (k_order_*) in their place
ALSO=k_nn_red; [ "$SF_REGS_SRC" == sf_icp.hip ] && ALSO=k_order
/opt/rocm/bin/hipcc "$@" -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -I../../include -I. -Rpass-analysis=kernel-resource-usage -c "$SRC" -o /tmp/kernel_regs.o 2>&1 |
  python3 -c "
import sys, re
name = None
for l in sys.stdin:
    m = re.search(r'Function Name: (\S+)', l)
    if m: name = m.group(1); d = {}
    for key in ('VGPRs', 'Occupancy \[waves/SIMD\]', 'SGPRs Spill', 'ScratchSize \[bytes/lane\]', 'LDS Size \[bytes/block\]'):
        m = re.search(key + r': (\d+)', l)
        if m and name: d[key] = m.group(1)
    if name and 'LDS Size' in l and any(k in name for k in ('$ALSO', 'k_nn_red', 'k_nn_deferred', 'k_ref_nn', 'k_ref_fused', 'k_bf', 'k_map_nn', 'k_icp_fused', 'k_nn_cov', 'k_cov_solve', 'k_normals', 'k_patch_old', 'k_map_knn', 'k_normals_knn', 'k_knn_mean_dist', 'k_tree_sum', 'k_flag_mean_dist', 'k_sum_kept', 'k_radius_count', 'k_rad_', 'k_cluster', 'k_plane', 'k_box', 'k_flag_boxes', 'k_reg_', 'k_iss_', 'k_features_gather', 'k_ndt_', 'k_ri_', 'k_vis_', 'k_sc_')):
        short = re.sub(r'^_ZN12_GLOBAL__N_1\d+', '', name)[:$WIDTH]
        print(short, 'vgpr', d.get('VGPRs'), 'occ', d.get('Occupancy \[waves/SIMD\]'), 'sgpr-spill', d.get('SGPRs Spill'), 'scratch', d.get('ScratchSize \[bytes/lane\]'), 'lds', d.get('LDS Size \[bytes/block\]'))
"
