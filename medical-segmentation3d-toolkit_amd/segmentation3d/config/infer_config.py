"""Default inference configuration -- same sections and keys as the reference's config/infer_config.py:9-113
(general / coarse / fine).  Copied next to trained models by `seg_train` and read back by `load_models`."""
#
# Optional keys of a stage section (coarse / fine), read with defaults so that they may be absent; add them to the
# infer_config.py of a model folder (they are not set here: this file keeps exactly the reference's keys):
#   blend_mode = 'constant'        'constant' | 'gaussian': weight of a patch voxel when overlapping patches are averaged
#   blend_sigma_scale = 0.125      Gaussian sigma as a fraction of the patch edge
#   tta_mirror_axes = []           e.g. ['x', 'y']: mirror test-time augmentation, 2^k forwards per patch
#   checkpoint = 'latest'          'latest' (largest chk_<n>) | 'best' (checkpoints/best of a run with validation) | an epoch
from easydict import EasyDict as edict

__C = edict()
cfg = __C

__C.general = {}
__C.general.single_scale = 'DISABLE'                   # 'coarse' | 'fine' | 'DISABLE' (= coarse-to-fine cascade)

__C.coarse = {}
__C.coarse.model_name = 'coarse'
__C.coarse.pick_largest_cc = True
__C.coarse.remove_small_cc = 0
__C.coarse.partition_type = 'DISABLE'                  # whole volume in one pass
__C.coarse.partition_size = [51.2, 51.2, 51.2]         # mm
__C.coarse.partition_stride = [51.2, 51.2, 51.2]
__C.coarse.cpu_model_spacing_increase_ratio = 1.0
__C.coarse.cpu_partition_decrease_ratio = 1.0

__C.fine = {}
__C.fine.model_name = 'fine'
__C.fine.pick_largest_cc = True
__C.fine.remove_small_cc = 0
__C.fine.partition_type = 'SIZE'                       # sliding window
__C.fine.partition_size = [96.0, 96.0, 96.0]           # mm
__C.fine.partition_stride = [48.0, 48.0, 48.0]
__C.fine.cpu_model_spacing_increase_ratio = 1.0
__C.fine.cpu_partition_decrease_ratio = 1.0
