"""flvis_amd -- MI355X-native (gfx950) FLVIS front-end tracking + local-map BA hot path.

Thin ctypes binding over the C ABI in include/flvis_hip.h (libflvis_hip.so, hand-written HIP kernels).  PyTorch is
used only as plumbing (device buffers, streams).  There is NO CPU fallback: without a HIP device every call raises.

One module per object; this file only gathers their names.  The C signatures are read from the header (_abi) and set once when
the library is loaded (_loader): a new entry point is declared in the header, and the signature follows.
"""
from ._loader import (FLVIS_ERR_CAPACITY, FLVIS_ERR_CONFIG, FLVIS_ERR_INVALID_ARG, FLVIS_ERR_NO_DEVICE, FLVIS_OK,  # noqa: F401
                      FlvisError, _P, _ptr, lib_path, load_library)
from ._structs import (FLVIS_LC_ALL_MAPS, FLVIS_LC_FIX_CAND, LC_ROW_WIDTH, LC_ROWS_IMU11, LC_ROWS_POSE8, LC_ROWS_TRAJ9,  # noqa: F401
                       LC_TRAJ_ANCHOR, LC_TRAJ_BLEND, FlvisCfg, FlvisImage, FlvisKeyframe, FlvisLcFix, FlvisLcFixIn, FlvisLcLink,
                       FlvisLcLinkQuery, FlvisLcMerge, FlvisLcTrajJob, FlvisStep, FrameOut, LcEvent, LcParams, OrbParams,
                       VocTrainParams, config_get_bool, load_config, load_lc_params, orb_default_pattern,
                       DepthCloudParams, depth_cloud_params, octomap_feeder_params, DenseStereoParams, dense_stereo_params,
                       OccupancyParams, occupancy_params, OccupancyCastParams, occupancy_cast_params)
from ._vocfile import TrainedVocabulary, convert_vocabulary_file, read_vocabulary_file, save_vocabulary_file  # noqa: F401
from ._context import OCCUPANCY_CAST_STATUS, Context, occupancy_info, voxel_cloud_info  # noqa: F401
from ._loop_closer import LoopCloser, _link_dict, links_from_fix, links_reverse, loop_candidate  # noqa: F401
from ._tracker import Tracker  # noqa: F401
