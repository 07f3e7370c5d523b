"""xchu_slam_amd — MI355X-native NDT scan-matching path of lowmee/xchu_slam (odom_node's registration step).

Product = libndt_hip.so (HIP kernels for gfx950 behind the C-ABI in include/ndt_hip.h) + this thin
host mirror of the pclomp::NormalDistributionsTransform API.  See DESIGN.md.
"""
from .odom import LidarOdom  # noqa: F401
from .icp import IterativeClosestPoint, refine_loop  # noqa: F401
from .gicp import GeneralizedIterativeClosestPoint  # noqa: F401
from .scancontext import SCManager, close_loops, detect_loops  # noqa: F401
from .isc import ISCGeneration, detect_loops_isc  # noqa: F401
from .posegraph import PoseGraph, gps_factors, loop_measurement, optimize_loops  # noqa: F401
from .globalmap import KeyframeMap, read_g2o, read_pcd, save_map, write_g2o, write_pcd, write_tum  # noqa: F401
from .pgo_node import PGO, detect_loop_radius, keyframe_gate, run_mapping  # noqa: F401
from .trajectory import ape, rpe  # noqa: F401
from .ground import CloudFilter, GroundResult, detect_ground  # noqa: F401
from .ndt import (DIRECT1, DIRECT7, DIRECT26, KDTREE, CpuNormalDistributionsTransform, NormalDistributionsTransform,  # noqa: F401
                  as_points, filter_scan, voxel_downsample)

__version__ = "0.1.0"
